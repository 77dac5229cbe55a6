"""The table of the host-path sweep (tests/test_gpu_hostpath_sweep.py), a numpy restatement of the
layout work the host-buffer entry points do around the chain, and a Python restatement of the rule
by which host_chain (radar-signal-process_amd/csrc/rsp_host.cpp) picks a route.  No GPU code and no
torch: tests/test_hostpath_cases_cpu.py holds all of it to a stand-alone program over rsp_hostplan.h
(tests/native/hostplan_cases.cpp).

Contexts are case_spec's of the MTD sweep: one matched-filter segment over the whole row,
R_out = R, any pin and R.  The four designed shapes:

  s1  48 x 69          V and R no multiples of 32, V R = 3312 a multiple of 4 (radix MTD)
  s2  33 x 69          Bluestein; V R = 2277 is odd, so one CPI with a row-major output is not
                       one-chunk eligible while a column-major output is
  s3  1024 x 517       a column-major one-chunk input goes in pieces of 128, 128, 128, 128, 5 rows
                       (fp16: 256, 256, 5), the column-major RDM comes back as 288 + 229 range bins,
                       the row-major one as spans of 265 216 and 264 192 cells; on the ring with one
                       CPI per chunk every 4.2 MB chunk goes in 4 DMA pieces
  s4  two beams        the smallest two-beam case of mtd_ref.CASES (300 pulses padded to 512 rows
                       x 21): batch * 2 input planes

The routes (route() below; the rule is host_chain's and zc_eligible's):

  one     nk == 1 and dbytes <= kZcMaxIn and nout * batch <= kParts and (out_tr or ocells % 4 == 0)
  chunk   the ring, because set_host_pipeline(chunk < batch) makes nk > 1
  odd     the ring, one host chunk, because ocells % 4 != 0 with a row-major output
  parts   the ring, one host chunk, because nout * batch > kParts = 16

Every case of the table fails at most one of the conditions, so its route has one reason
(test_hostpath_cases_cpu.py).

Layout instances of rsp_layout.hip that no entry point reaches: host_chain narrows C128 to C64 on
the copy threads before anything lands on the device (ddtype is never RSP_C128) and calls
launch_canon only for a column-major input, so ingest_row_kernel<float2>, <double2> and <__half2>
(launch_canon's row-major branch) and transpose_kernel<double2, float2> (its RSP_C128 branch) are
compiled but never launched.  The sweep cannot visit them and does not count them.
"""
import dataclasses

import numpy as np

import mtd_ref as mr

C64, C128, F16 = 0, 1, 2           # rsp_dtype: RSP_C64, RSP_C128, RSP_C32F16
ROW, COL = 0, 1                    # rsp_layout
DTYPE_NAME = {C64: "c64", C128: "c128", F16: "f16"}
LAYOUT_NAME = {ROW: "row", COL: "col"}

# rsp_hostplan.h
K_HOST_CHUNK_BYTES = 32 << 20
K_ZC_MAX_IN = 64 << 20
K_PARTS = 16

ROUTES = ("one", "chunk", "odd", "parts")
SEED = 20250317


# ------------------------------------------------------------------------------------- shapes
@dataclasses.dataclass(frozen=True)
class Shape:
    id: str
    pin: int
    R: int
    nfft: int = 0
    beams: int = 1

    @property
    def V(self):
        return self.nfft or self.pin

    @property
    def cells(self):
        return self.V * self.R


def _smallest_two_beam():
    c = min((c for c in mr.CASES if c.beams == 2), key=lambda c: (c.pin * c.R, c.V))
    return Shape("s4", c.pin, c.R, c.nfft, 2)


SHAPES = {s.id: s for s in (Shape("s1", 48, 69), Shape("s2", 33, 69), Shape("s3", 1024, 517), _smallest_two_beam())}


# -------------------------------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    """One host call of the sweep.  entry: "chain" (rsp_pc_mtd_cfar, or rsp_pc_mtd_cfar_f64 with
    f64) or "pc_mtd" (the forwarding wrapper).  nout: 1 RDM, 2 RDM + flag, 3 RDM + flag + flagV.
    chunk: set_host_pipeline's CPIs per chunk (0: by size).  want: the route the case is designed
    to take."""
    shape: str
    want: str
    batch: int
    chunk: int
    dtype: int
    layout: int
    out_layout: int
    f64: bool
    nout: int
    entry: str = "chain"

    @property
    def id(self):
        return "%s-%s-b%dk%d-%s%s-%s%s%d%s" % (
            self.shape, self.want, self.batch, self.chunk, DTYPE_NAME[self.dtype], LAYOUT_NAME[self.layout],
            LAYOUT_NAME[self.out_layout], "f64" if self.f64 else "f32", self.nout, "-pcmtd" if self.entry == "pc_mtd" else "")

    @property
    def group(self):
        return "%s-%s" % (self.shape, self.want)


INPUTS = [(d, lay) for d in (C128, C64, F16) for lay in (ROW, COL)]
OUTPUTS = [(ol, f64, nout) for ol in (ROW, COL) for f64 in (False, True) for nout in (1, 2, 3)]


def _plan(shape, want, out_layout, nout):
    """(batch, chunk) with which a call of `shape` takes route `want`, or None where it cannot."""
    if want == "chunk":
        return 5, 2                                   # chunks of 2, 2 and 1 CPIs: slot 0 is reused
    if want == "parts":                               # nout * batch = 20, 24, 24 > 16
        return (20, 12, 8)[nout - 1], 0
    if shape == "s2":                                 # 2277 cells per CPI
        if want == "odd":
            return (1, 0) if out_layout == ROW else None
        return (4, 0) if out_layout == ROW else (1, 0)     # 9108 cells in rows; one CPI in columns
    if want == "odd":
        return None
    return 2, 0


def _product(shape):
    out = []
    for want in ROUTES:
        for d, lay in INPUTS:
            for ol, f64, nout in OUTPUTS:
                p = _plan(shape, want, ol, nout)
                if p:
                    out.append(Case(shape, want, p[0], p[1], d, lay, ol, f64, nout))
    return out


def _pairwise(shape, want, batch, chunk, outputs, turns=1):
    """Every (dtype, layout) of the input with `turns` of the outputs each, walking through them."""
    out = []
    for i, (d, lay) in enumerate(INPUTS):
        for t in range(turns):
            ol, f64, nout = outputs[(i + t * len(INPUTS)) % len(outputs)]
            b = batch[nout - 1] if isinstance(batch, tuple) else batch
            out.append(Case(shape, want, b, chunk, d, lay, ol, f64, nout))
    return out


def _cases():
    out = _product("s1") + _product("s2")
    three = [o for o in OUTPUTS if o[2] == 3]
    # s3: every output combination on the one-chunk route (6 inputs x 2), half of them on the ring
    # with one 4.2 MB CPI per chunk (3 chunks); 6 CPIs with three outputs for the 16-part limit
    out += _pairwise("s3", "one", 1, 0, OUTPUTS, turns=2)
    out += _pairwise("s3", "chunk", 3, 1, OUTPUTS[1::2] + OUTPUTS[0::2])
    out += [Case("s3", "parts", 6, 0, C64, COL, COL, False, 3), Case("s3", "parts", 6, 0, F16, ROW, ROW, True, 3)]
    # s4: two beams
    out += _pairwise("s4", "one", 1, 0, OUTPUTS, turns=2)
    out += _pairwise("s4", "chunk", 5, 2, OUTPUTS[1::2] + OUTPUTS[0::2])
    out += _pairwise("s4", "parts", 6, 0, three + three)
    # rsp_pc_mtd forwards to rsp_pc_mtd_cfar: one call per route it can take and per layout pair
    for want in ("one", "chunk", "parts"):
        b, k = _plan("s1", want, ROW, 1)
        out += [Case("s1", want, b, k, C128, COL, COL, False, 1, "pc_mtd"),
                Case("s1", want, b, k, C64, ROW, ROW, False, 1, "pc_mtd")]
    out.append(Case("s2", "odd", 1, 0, C128, COL, ROW, False, 1, "pc_mtd"))
    return out


CASES = _cases()
GROUPS = sorted({c.group for c in CASES})

# rsp_cfar / rsp_cfar_f64 on the device path's RDM: (shape, batch).  s2 with one CPI in rows is
# 2277 cells: rsp_cfar_f64 leaves its one-chunk path for the ring there.
CFAR_CALLS = [("s1", 1), ("s1", 4), ("s2", 1), ("s2", 4)]


# -------------------------------------------------------------------------------------- route
def dev_elem_size(dtype):
    """Bytes per sample on the device: C128 is narrowed to C64 by the copy threads."""
    return 4 if dtype == F16 else 8


def host_chunks(batch, host_chunk, dev_cpi):
    """rsp_hostplan.h host_chunks: (K, nk, [size of each chunk])."""
    K = host_chunk if host_chunk > 0 else K_HOST_CHUNK_BYTES // max(dev_cpi, 1)
    K = max(1, min(K, batch))
    nk = (batch + K - 1) // K
    return K, nk, [batch - k * K if k == nk - 1 else K for k in range(nk)]


def route(case):
    """dict(route, eligible, K, nk, sizes, reasons): which of ROUTES host_chain takes for the call,
    whether zc_eligible holds, its host chunks, and the conditions of zc_eligible that fail
    (host_chain asks only when nk == 1: with more chunks the route is "chunk" whatever they say)."""
    s = SHAPES[case.shape]
    dev_cpi = s.beams * s.pin * s.R * dev_elem_size(case.dtype)
    dbytes = case.batch * dev_cpi
    ocells = case.batch * s.V * s.R
    K, nk, sizes = host_chunks(case.batch, case.chunk, dev_cpi)
    in_tr, out_tr = case.layout == COL, case.out_layout == COL
    why = []
    if case.nout * case.batch > K_PARTS:
        why.append("parts")
    if not (out_tr or ocells % 4 == 0):
        why.append("odd")
    if dbytes > K_ZC_MAX_IN or not (in_tr or dbytes % 4 == 0):
        why.append("size")
    r = "chunk" if nk > 1 else (why[0] if why else "one")
    return dict(route=r, eligible=not why, K=K, nk=nk, sizes=sizes, reasons=why)


def census(cases):
    """{route: (inputs seen, outputs seen)} by route() of every case."""
    seen = {r: (set(), set()) for r in ROUTES}
    for c in cases:
        ins, outs = seen[route(c)["route"]]
        ins.add((c.dtype, c.layout))
        outs.add((c.out_layout, c.f64, c.nout))
    return seen


def expected_census():
    """Every input form and every output combination on every route; the route "odd" exists only
    with a row-major output."""
    return {r: (set(INPUTS), {o for o in OUTPUTS if r != "odd" or o[0] == ROW}) for r in ROUTES}


def native_args(case):
    """The case as tests/native/hostplan_cases.cpp's argv."""
    s = SHAPES[case.shape]
    return [str(v) for v in (case.batch, case.chunk, s.beams, s.pin, s.R, s.V, s.R, dev_elem_size(case.dtype),
                             int(case.layout == COL), int(case.out_layout == COL), case.nout)]


# --------------------------------------------------------------------------------- layout work
def expected_outputs(rdm, flag, flagV, out_layout, f64):
    """What a host call must return for the device path's row-major planes [batch, V, R]: the
    caller's layout (column-major: [batch, R, V]) and type (f64: every plane widened, exactly)."""
    out = []
    for a in (rdm, flag, flagV):
        if a is None:
            continue
        if out_layout == COL:
            a = np.swapaxes(a, -1, -2)
        out.append(np.ascontiguousarray(a.astype(np.float64) if f64 else a))
    return tuple(out)


def to_half_iq(echo64):
    """complex64 [...] -> float16 [..., 2] I/Q pairs (round to nearest even)."""
    return np.ascontiguousarray(np.stack([echo64.real, echo64.imag], axis=-1).astype(np.float16))


def echo_variants(echo64):
    """{(dtype, layout): array} of a complex64 echo [..., P, R]: itself, its exact widening to
    complex128, the fp16 I/Q form [..., P, R, 2], and the column-major form of each (MATLAB's P x R
    array is numpy's C-ordered [..., R, P]; fp16: [..., R, P, 2])."""
    e = np.ascontiguousarray(echo64, dtype=np.complex64)
    half = to_half_iq(e)
    return {(C64, ROW): e, (C64, COL): np.ascontiguousarray(np.swapaxes(e, -1, -2)),
            (C128, ROW): e.astype(np.complex128), (C128, COL): np.ascontiguousarray(np.swapaxes(e, -1, -2).astype(np.complex128)),
            (F16, ROW): half, (F16, COL): np.ascontiguousarray(np.swapaxes(half, -2, -3))}


def noise_echo(shape, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(0.5)).astype(np.complex64)


TIE_DOWN, TIE_UP = 1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24      # fp32 round-to-even ties
PLANTED = ((TIE_DOWN, np.float32(1.0)), (TIE_UP, np.float32(1.0 + 2.0 ** -22)), (-TIE_DOWN, np.float32(-1.0)),
           (-TIE_UP, np.float32(-1.0 - 2.0 ** -22)), (1e-60, np.float32(0.0)), (-1e-50, np.float32(0.0)))


def planted_at(n):
    """Flat indices of the planted values in an echo of n samples: both ends, and a walk between."""
    k = len(PLANTED)
    return [0, n - 1] + [(i * n) // (2 * k - 1) + 1 for i in range(1, 2 * k - 1)]


def double_echo(shape, seed):
    """A complex128 echo that is not float-representable: double noise, with the values of PLANTED
    in the real and (in turn) imaginary parts at planted_at().  Its C64 form is astype(complex64)."""
    rng = np.random.default_rng(seed)
    e = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(0.5)
    flat = e.reshape(-1).view(np.float64).reshape(-1, 2)
    for i, at in enumerate(planted_at(flat.shape[0])):
        flat[at, i % 2] = PLANTED[i % len(PLANTED)][0]
    return e


def column_major_c128(echo128):
    return np.ascontiguousarray(np.swapaxes(echo128, -1, -2))


# ------------------------------------------------------------------------------------- guards
SENTINEL = 0xA5
GUARD = 4096


def guarded(shape, dtype, lead=GUARD):
    """(raw, view): a uint8 buffer of SENTINEL bytes and the array of `shape` inside it, `lead`
    bytes from its start and at least GUARD bytes from its end."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    assert lead >= GUARD and lead % np.dtype(dtype).itemsize == 0
    raw = np.full(lead + n + GUARD, SENTINEL, np.uint8)
    return raw, raw[lead:lead + n].view(dtype).reshape(shape)


def guards_intact(raw, view, lead=GUARD):
    n = view.nbytes
    return bool((raw[:lead] == SENTINEL).all() and (raw[lead + n:] == SENTINEL).all())
