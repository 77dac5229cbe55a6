"""Pulse compression across its dispatch table, per segment, against fp64.

At context creation the host picks a pulse-compression path from the segment lengths alone: the
generic pc_kernel, one of nine single-length pc_mf_kernel instances, one of five fused pairs, one
of two pruned instances of the 1024/4096 pair, or an overlap-save split into 2048-, 4096- or
8192-point blocks.  Every row of CASES is one geometry chosen to sit on a boundary of those
rules, with the plan it must select (rsp_pc_plan; worked out by hand from pc_overlap_save,
pc_prune_counts, pc_fused and pc_prune_select, never copied from the library's answer).

Each case runs Engine.pc_dev into the middle of a NaN-filled buffer and is compared, segment by
segment, with an fp64 restatement of the segment contract of include/rsp.h (rsp_seg_kind):

  MF   ifft(fft(x[in], nfft) * conj(fft(scale * coef, nfft)))[:out_len]
  FIR  scale * filter(taps, 1, x[in]), rolled left by fir_shift mod len
  columns no segment covers: exactly 0

test_reference_matches_oracle pins that restatement to the oracle's fun_lss_pulse_compression.

Row counts: 6 rows (P = 3, batch 2) where every transform has 1024 points or more (4 or 1 rows
per workgroup), 74 rows (P = 37) where one has 512 or fewer (up to 64 rows per workgroup) -- more
than one workgroup and a partly filled last one either way.
"""
import numpy as np
import pytest

import rsp_ref as ref
from _util import MAX_TOL, RDM_TOL

FIR, MF = 0, 1     # rsp_seg_kind
SEED = 20240611


# ------------------------------------------------------------------------------- fp64 reference
def ref_pc(spec, x):
    """x: [rows, R] complex128 -> [rows, R_out] complex128 by the segment contract."""
    out = np.zeros((x.shape[0], spec.pc_width or spec.R_out), np.complex128)
    for s in spec.segments:
        xin = x[:, s.in_start:s.in_start + s.in_len]
        if s.kind == FIR:
            z = s.scale * ref.mfilter(np.real(s.coef), xin)
            y = np.roll(z, -(s.fir_shift % s.in_len), axis=-1)
        else:
            H = np.conj(np.fft.fft(s.scale * np.asarray(s.coef, np.complex128), s.nfft))
            y = np.fft.ifft(np.fft.fft(xin, s.nfft, axis=-1) * H, axis=-1)[:, :s.out_len]
        out[:, s.out_start:s.out_start + s.out_len] = y
    return out


def uncovered(spec):
    m = np.ones(spec.pc_width or spec.R_out, bool)
    for s in spec.segments:
        m[s.out_start:s.out_start + s.out_len] = False
    return m


@pytest.mark.parametrize("pp", [[2600, 100, 400, 1500], [2600, 17, 768, 1815], [2600, 1051, 314, 1000]])
def test_reference_matches_oracle(pp):
    """ref_pc on a v2 spec against rsp_ref.fun_lss_pulse_compression.  Both are fp64; they differ
    in the FFT length (nextpow2 against the exact linear length), so by a few eps * log2(N) ~ 1e-15
    of the segment's scale: 1e-12 leaves three decades.  The tail past p3 is 0 in both."""
    from rsp import presets
    P, R = 2, pp[0]
    spec = presets.v2(P, R, point_prt=pp)
    rng = np.random.default_rng(SEED)
    x = rng.standard_normal((P, R)) + 1j * rng.standard_normal((P, R))
    _, p2, p3 = ref.v2_pulses(ref.v2_params(P, R, pp))
    want = ref.fun_lss_pulse_compression(x, p2, p3, pp[1], pp[2], pp[3], fir_shift=True)
    got = ref_pc(spec, x)
    assert np.max(np.abs(got - want)) / np.max(np.abs(want)) < 1e-12
    tail = uncovered(spec)
    assert tail.sum() == R - sum(pp[1:]) and not got[:, tail].any() and not want[:, tail].any()


# ------------------------------------------------------------------------------------ the table
def seg(nfft, zin=0, zout=0, nsub=0, step=0, fir=0):
    return (nfft, nsub, step, zin, zout, fir)


GENERIC = dict(specialised=0, fused=0, prune=0, segs=[])


def plan(fused, prune, *segs):
    return dict(specialised=1, fused=fused, prune=prune, segs=list(segs))


class Case:
    def __init__(self, cid, build, want, whole=None, var=""):
        self.id, self.build, self.plan, self.whole, self.var = cid, build, want, whole, var


def v2_spec(p1, p2, m3, p3, nfft3=None):
    def build(P):
        from rsp import presets
        R = p1 + p2 + m3
        spec = presets.v2(P, R, point_prt=[R, p1, p2, p3])
        if nfft3:
            spec.segments[2].nfft = nfft3
        return spec
    return build


def seg_spec(R, R_out, segs):
    """segs: (kind, in_start, in_len, out_start, out_len, nfft, replica length) -- the DMX replica
    (67 samples, or its first n) for a matched filter, the raw 35 taps for a FIR."""
    def build(P):
        from rsp import presets
        rep = presets.dmx_replica()
        out = []
        for kind, i0, il, o0, ol, nfft, n in segs:
            if kind == FIR:
                out.append(presets.Segment(FIR, i0, il, o0, ol, presets.FIR_TAPS / presets.FIR_TAPS.max(),
                                           scale=1.0 / 1.2, fir_shift=17))
            else:
                out.append(presets.Segment(MF, i0, il, o0, ol, rep[:n], nfft=nfft))
        return presets.Spec("geom", P, R, R_out, out, cfar_segments=[(0, R_out)],
                            radar=presets.radar_params(P, R))
    return build


def V2(cid, p1, p2, m3, p3, fused, prune, s2, s3, whole=None, var="", nfft3=None):
    """v2 geometry: pulses of 200 and 700 samples, nfft2 = nextpow2(p2 + 199), nfft3 =
    nextpow2(m3 + 699); s2 = (nfft, z) with zin = zout = z, the FIR riding on it."""
    w = None
    if whole:
        wf, wp, ws3 = whole
        w = plan(wf, wp, seg(s2[0], s2[1], s2[1], fir=1), ws3)
    return Case(cid, v2_spec(p1, p2, m3, p3, nfft3), plan(fused, prune, seg(s2[0], s2[1], s2[1], fir=1), s3),
                w, var)


def single(cid, nfft, in_len, out_len, want, whole=None, var="", rep=67):
    return Case(cid, seg_spec(in_len, out_len, [(MF, 0, in_len, 0, out_len, nfft, rep)]), plan(0, 0, want),
                plan(0, 0, whole) if whole else None, var)


S1K4 = (1024, 4)   # 723 or 768 of 1024 points: (1024 - 768) / 64 = 4 slices
CASES = [
    # ---- (a) the pruned pair's predicate: zin1, zout1 >= 4, then (zin2, zout2) >= (3, 3) or zout2 >= 2
    V2("a-4433-zero-slack", 228, 768, 3328, 3328, 1, 0x4433, S1K4, seg(4096, 3, 3), var="hg"),
    V2("a-zin1-3-generic-pair", 228, 769, 3328, 3328, 1, 0, (1024, 3), seg(4096, 3, 3)),
    V2("a-4402-whole-row", 228, 768, 3329, 3329, 1, 0x4402, S1K4, seg(4096, 2, 2), var="h"),
    V2("a-4402-whole-row-max", 228, 768, 3397, 3397, 1, 0x4402, S1K4, seg(4096, 2, 2), var="g"),
    V2("a-zin2-zout3", 228, 768, 3329, 3328, 1, 0x4402, S1K4, seg(4096, 2, 3)),
    V2("a-15-out-slices-cut", 228, 768, 3328, 100, 1, 0x4433, S1K4, seg(4096, 3, 15), var="h"),
    V2("a-shortest-1024-4096", 228, 314, 1350, 1350, 1, 0x4433, (1024, 11), seg(4096, 10, 10), var="g"),
    V2("a-slice-edge-3072", 228, 768, 3072, 3072, 1, 0x4433, S1K4, seg(4096, 4, 4)),
    V2("a-slice-edge-3073", 228, 768, 3073, 3073, 1, 0x4433, S1K4, seg(4096, 3, 3)),
    # ---- (b) FIR edges: shorter than the 17-sample shift, than the 35 taps; 1050 + 39 staged
    #      samples fill the 1089-sample slot of a 1024-point row, 1051 fall back to pc_kernel
] + [
    V2("b-fir-%d" % p1, p1, 400, 1500, 1500, 1, 0x4433, (1024, 9), seg(4096, 10, 10), var=v)
    for p1, v in ((1, "g"), (16, ""), (17, "h"), (18, ""), (34, "g"), (35, ""), (36, ""), (1050, "hg"))
] + [
    Case("b-generic-1051", v2_spec(1051, 314, 1000, 1000), GENERIC, var="h"),
    Case("b-generic-zero-tail", v2_spec(2000, 300, 1500, 1000), GENERIC),
    V2("b-fir-on-256", 100, 40, 900, 900, 0, 0, (256, 0), seg(2048, 8, 8), var="hg"),
    # ---- (c) pairs and non-pairs
    V2("c-1024-2048-unfused", 228, 723, 1349, 1349, 0, 0, S1K4, seg(2048, 5, 5), var="g"),
    V2("c-512-4096-unfused", 100, 300, 3000, 3000, 0, 0, (512, 0), seg(4096, 4, 4), var="h"),
    V2("c-pair-512-1024", 82, 300, 325, 325, 1, 0, (512, 0), seg(1024, 10, 10), var="hg"),
    V2("c-pair-1024-1024", 228, 723, 73, 73, 1, 0, S1K4, seg(1024, 14, 14)),
    Case("c-three-mf", seg_spec(2300, 2300, [(MF, 0, 100, 0, 100, 128, 67), (MF, 100, 400, 100, 400, 512, 67),
                                             (MF, 500, 1800, 500, 1800, 2048, 67)]),
         plan(0, 0, seg(128), seg(512), seg(2048, 1, 1)), var="g"),
    # ---- (d) overlap-save: blocks of nb points keep nb - 699 outputs (3397 of 4096, 1349 of 2048,
    #      7493 of 8192); the fewest transformed points win, the longer block on a tie
    #      3398 outputs: 3 x 2048 (6144 points) beat 2 x 4096 -- and 1024 + 2048 is no built pair
    V2("d-3398", 228, 723, 3398, 3398, 0, 0, S1K4, seg(2048, 0, 5, 3, 1349),
       whole=(1, 0, seg(8192, 9, 9)), var="h"),
    V2("d-6794-two-full-steps", 228, 723, 6794, 6794, 1, 0x4402, S1K4, seg(4096, 0, 2, 2, 3397),
       whole=(1, 0, seg(8192, 2, 2)), var="g"),
    V2("d-6795-last-block-1-output", 228, 723, 6795, 6795, 1, 0x4402, S1K4, seg(4096, 0, 2, 3, 3397),
       whole=(1, 0, seg(8192, 2, 2)), var="h"),
    V2("d-7493", 228, 723, 7493, 7493, 1, 0x4402, S1K4, seg(4096, 0, 2, 3, 3397),
       whole=(1, 0, seg(8192, 1, 1))),
    V2("d-nsub1-in-7000", 228, 723, 7000, 3397, 1, 0x4402, S1K4, seg(4096, 0, 2, 1, 3397),
       whole=(1, 0, seg(8192, 2, 9)), var="hg"),
    V2("d-7494", 228, 723, 7494, 7494, 1, 0x4402, S1K4, seg(4096, 0, 2, 3, 3397),
       whole=(1, 0, seg(16384, 8, 8))),
    V2("d-14986-blocks-8192", 228, 723, 14986, 14986, 1, 0, S1K4, seg(8192, 0, 1, 2, 7493),
       whole=(1, 0, seg(16384, 1, 1)), var="hg"),
    V2("d-14987", 228, 723, 14987, 14987, 1, 0x4402, S1K4, seg(4096, 0, 2, 5, 3397),
       whole=(1, 0, seg(16384, 1, 1))),
    single("d-one-2048-block", 8192, 8000, 1900, seg(2048, 0, 1, 1, 1982), whole=seg(8192, 0, 12), var="g"),
    #      a forced 8192-point third segment of 3000 samples: one 4096-point block whose input ends
    #      before slice 12 -- the (4,4,3,3) instance behind overlap-save
    V2("d-4433-behind-ols", 228, 723, 3000, 3000, 1, 0x4433, S1K4, seg(4096, 4, 4, 1, 3397),
       whole=(1, 0, seg(8192, 10, 10)), var="h", nfft3=8192),
]

# ---- (e) single segments, no FIR: circular (in = out = nfft, which never splits: the outputs wrap)
#      and cut (in = nfft - nfft/16 - 1, out = nfft/16 + 1; above 4096 points that is one
#      2048-point overlap-save block of 1982 outputs)
for _n, _vc, _vk in ((64, "h", "g"), (128, "g", "h"), (256, "hg", ""), (512, "", "hg"), (1024, "h", "g"),
                     (2048, "g", "h"), (4096, "", "hg"), (8192, "h", ""), (16384, "g", "h")):
    _g, _rep = _n // 16, 40 if _n == 64 else 67
    CASES.append(single("e-%d-circular" % _n, _n, _n, _n, seg(_n), var=_vc, rep=_rep))
    _z = (1, 14) if _n >= 1024 else (0, 0)   # (g + 1) // g and (15 g + 1) // g slices
    if _n <= 4096:
        CASES.append(single("e-%d-cut" % _n, _n, _n - _g - 1, _g + 1, seg(_n, *_z), var=_vk, rep=_rep))
    else:   # zout = (2048 - 513) // 128, (2048 - 1025) // 128
        CASES.append(single("e-%d-cut" % _n, _n, _n - _g - 1, _g + 1,
                            seg(2048, 0, 11 if _n == 8192 else 7, 1, 1982), whole=seg(_n, *_z), var=_vk))
for _n in (1024, 4096):
    _g = _n // 16
    _zs = {1: 15, _g - 1: 15, _g: 15, _g + 1: 14}   # (n - v) // g
    for _i, _o, _v in ((1, 1, ""), (_g - 1, _g - 1, ""), (_g, _g, ""), (_g + 1, _g + 1, "g" if _n == 1024 else "h"),
                       (1, _g + 1, ""), (_g + 1, 1, "")):
        CASES.append(single("e-%d-in%d-out%d" % (_n, _i, _o), _n, _i, _o, seg(_n, _zs[_i], _zs[_o]), var=_v))

# ---- (f) uncovered output columns without a FIR to write them (and one with, as the control)
CASES += [
    Case("f-one-mf-gaps", seg_spec(1000, 600, [(MF, 5, 900, 10, 500, 1024, 67)]),
         plan(0, 0, seg(1024, 1, 8)), var="hg"),
    Case("f-two-mf-gap7", seg_spec(1000, 1007, [(MF, 0, 300, 0, 300, 512, 67), (MF, 300, 700, 307, 700, 1024, 67)]),
         plan(1, 0, seg(512), seg(1024, 5, 5)), var="g"),
    Case("f-fir-two-mf-gap7", seg_spec(1082, 1089, [(FIR, 0, 82, 0, 82, 0, 0), (MF, 82, 300, 82, 300, 512, 67),
                                                    (MF, 382, 700, 389, 700, 1024, 67)]),
         plan(1, 0, seg(512, fir=1), seg(1024, 5, 5)), var="h"),
    #      9000 outputs of a 16384-point row: 5 x 2048 (1982 outputs each) is the fewest points
    Case("f-ols-zero-tail", seg_spec(15000, 9500, [(MF, 0, 15000, 0, 9000, 16384, 67)]),
         plan(0, 0, seg(2048, 0, 0, 5, 1982)), plan(0, 0, seg(16384, 1, 7)), var="hg"),
]

PARAMS = [pytest.param(c, v, id="%s-%s" % (c.id, v)) for c in CASES
          for v in ["c64"] + (["f16"] if "h" in c.var else []) + (["gain"] if "g" in c.var else [])]


def test_table_covers_every_path():
    """Every dispatch path appears in an asserted plan: the generic kernel, the nine single lengths,
    the five pairs (default or whole-transform plan), both pruned codes on a whole row and behind
    overlap-save, the three block lengths and a one-block split."""
    plans = [c.plan for c in CASES] + [c.whole for c in CASES if c.whole]
    assert any(not p["specialised"] for p in plans)
    singles = {p["segs"][0][0] for p in plans if p["specialised"] and len(p["segs"]) == 1}
    assert singles >= {64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384}
    pairs = {(p["segs"][0][0], p["segs"][1][0]) for p in plans if p["fused"]}
    assert pairs == {(1024, 1024), (1024, 4096), (1024, 8192), (1024, 16384), (512, 1024)}
    for code in (0x4433, 0x4402):
        assert any(p["prune"] == code and p["segs"][1][1] == 0 for p in plans), hex(code)
        assert any(p["prune"] == code and p["segs"][1][1] >= 1 for p in plans), hex(code)
    split = {(s[0], s[1] == 1) for p in plans for s in p["segs"] if s[1] >= 1}
    assert {n for n, _ in split} == {2048, 4096, 8192} and any(one for _, one in split)


# --------------------------------------------------------------------------------------- the run
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _no_prune(p):
    return dict(p, prune=0, segs=[(n, ns, st, 0, 0, f) for n, ns, st, _, _, f in p["segs"]])


def _seg_err(got, want, s):
    cols = slice(s.out_start, s.out_start + s.out_len)
    g, w = got[..., cols].astype(np.complex128), want[..., cols]
    return float(np.linalg.norm(g - w) / np.linalg.norm(w)), float(np.max(np.abs(g - w)) / np.max(np.abs(w)))


# Cases whose kept outputs are a vanishing part of what the transform computes, so that a bar taken
# relative to the kept columns measures the fp32 spectrum's rounding and not the kernel.  A single
# input sample x[0] leaves y[0] = x[0] conj(h[0]) as the only non-zero kept output (the other 66
# land at the end of the nfft-point row), and h[0], the Kaiser-windowed replica's edge, is 7.3e-4 of
# max|h|: the fp32 spectrum H alone (eps 6e-8 of max|H|) gives ~1e-4 of y[0].  A plain fp32 FFT
# of the same rows gives the same figures.  For these the issue's fallback holds: at most twice the
# generic instance's figure (prune off, split off), and -- the statement the kernel can be held to --
# max|d| under MAX_TOL of the whole nfft-point correlation's maximum (measured: 2.2e-8, 5.1e-8, 3.6e-8).
#   case                     default instance (rel, max)   generic instance (rel, max)
#   e-1024-in1-out1          2.34e-05, 3.07e-05            the same launch: 2.34e-05, 3.07e-05
#   e-1024-in1-out65         2.32e-04, 7.01e-05            the same launch: 2.32e-04, 7.01e-05
#   e-4096-in1-out257        2.90e-04, 5.00e-05            the same launch: 2.90e-04, 5.00e-05
# (a single-segment launch has no pruned instance and these rows no split: both columns are the
# same kernel; e-4096-in1-out1 stays under the bars at 8.6e-06, 8.9e-06)
ILL_CONDITIONED = ("e-1024-in1-out1", "e-1024-in1-out65", "e-4096-in1-out257")


def _run(torch, eng, d_in, batch):
    """pc_dev into CPIs [1, batch] of a NaN-filled [batch + 2] buffer; the guards must stay NaN."""
    P, W = eng.spec.P, eng.spec.pc_width or eng.spec.R_out
    buf = torch.full((batch + 2, P, W, 2), float("nan"), dtype=torch.float32, device="cuda")
    eng.pc_dev(d_in, torch.view_as_complex(buf)[1:batch + 1])
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.isnan(h[0]).all() and np.isnan(h[-1]).all(), "a guard CPI was written"
    return np.ascontiguousarray(h[1:-1]).view(np.complex64)[..., 0]


@pytest.mark.gpu
@pytest.mark.parametrize("case,variant", PARAMS)
def test_pc_geometry(torch_cuda, case, variant):
    from rsp import synth
    from rsp.engine import Engine
    torch = torch_cuda
    batch = 2
    probe = case.build(3)
    P = 37 if any(s.kind == MF and s.nfft <= 512 for s in probe.segments) else 3
    spec = case.build(P)
    R = spec.R
    rng = np.random.default_rng(SEED)
    echo = ((rng.standard_normal((batch, P, R)) + 1j * rng.standard_normal((batch, P, R))) * np.sqrt(0.5))
    echo = echo.astype(np.complex64)
    if variant == "f16":   # the reference sees the rounded fp16 values
        half = synth.to_half_iq(echo)
        x = half[..., 0].astype(np.float64) + 1j * half[..., 1].astype(np.float64)
        d_in = torch.from_numpy(half).cuda()
    else:
        x = echo.astype(np.complex128)
        d_in = torch.from_numpy(echo).cuda()
    with Engine(spec, device=0) as eng:
        if variant == "gain":   # fused iSTC: echo column n times gain[n]
            gain = np.linspace(0.5, 2.0, R).astype(np.float32)
            eng.set_prefilter(gain=gain)
            x = x * gain.astype(np.float64)
        assert eng.pc_plan() == case.plan
        got = _run(torch, eng, d_in, batch)
        assert np.isfinite(got.view(np.float32)).all(), "unwritten or non-finite output"
        want = ref_pc(spec, x.reshape(batch * P, R)).reshape(batch, P, -1)
        gap = uncovered(spec)
        assert not got[..., gap].any(), "uncovered columns are not 0"
        over = []
        for i, s in enumerate(spec.segments):
            err, emax = _seg_err(got, want, s)
            print("%s %s segment %d: rel %.3g max %.3g" % (case.id, variant, i, err, emax))
            if not (err < RDM_TOL and emax < MAX_TOL):
                over.append((i, s, err, emax))
        if over:   # only the recorded ill-conditioned cases, and only as far as the generic instance
            assert case.id in ILL_CONDITIONED, [(i, e, m) for i, _, e, m in over]
            eng.set_pc_prune(0)
            eng.set_pc_split(0)
            generic = _run(torch, eng, d_in, batch)
            eng.set_pc_prune(1)
            eng.set_pc_split(1)
            xr = x.reshape(batch * P, R)
            for i, s, err, emax in over:
                gerr, gmax = _seg_err(generic, want, s)
                print("%s %s segment %d: generic instance rel %.3g max %.3g" % (case.id, variant, i, gerr, gmax))
                assert err <= 2 * gerr and emax <= 2 * gmax, (i, err, emax, gerr, gmax)
                H = np.conj(np.fft.fft(s.scale * np.asarray(s.coef, np.complex128), s.nfft))
                full = np.fft.ifft(np.fft.fft(xr[:, s.in_start:s.in_start + s.in_len], s.nfft, axis=-1) * H, axis=-1)
                d = got[..., s.out_start:s.out_start + s.out_len].reshape(batch * P, -1) - full[:, :s.out_len]
                efull = float(np.max(np.abs(d)) / np.max(np.abs(full)))
                print("%s %s segment %d: max|d| / max|whole correlation| %.3g" % (case.id, variant, i, efull))
                assert efull < MAX_TOL, (i, efull)
        if case.plan["prune"]:   # the pruned instance against the generic one: equal value for value
            eng.set_pc_prune(0)
            assert eng.pc_plan() == _no_prune(case.plan)
            assert np.array_equal(got, _run(torch, eng, d_in, batch))
            eng.set_pc_prune(1)
        if case.whole:   # overlap-save against the whole-length transform
            eng.set_pc_split(0)
            assert eng.pc_plan() == case.whole
            whole = _run(torch, eng, d_in, batch)
            assert np.isfinite(whole.view(np.float32)).all()
            split = np.zeros(got.shape[-1], bool)
            for s, ps in zip([s for s in spec.segments if s.kind == MF], case.plan["segs"]):
                if ps[1] >= 1:
                    split[s.out_start:s.out_start + s.out_len] = True
            assert np.array_equal(got[..., ~split], whole[..., ~split])
            d = float(np.linalg.norm(got - whole) / np.linalg.norm(whole))
            assert d < 2e-6, d
