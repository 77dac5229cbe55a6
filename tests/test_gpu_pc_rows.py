"""Rows per workgroup of the 4096-point pulse-compression rows (rsp_set_pc_rows): 2 and 4 against 1.

With n = 2 or 4 a long-row workgroup runs n consecutive units (row, overlap-save block) in a loop
and loads the spectrum slice and twiddles once.  Each row's operations and their order are those
of one row per workgroup, so every stored value must keep its bits: the outputs are compared as
uint32 words, which also tells -0 from +0.  Each run writes into NaN-filled CPIs between two guard
CPIs of sentinel bytes, so a unit that stores where it should not, or not at all, shows.

The shapes are the smallest at which the row loop can go wrong: a workgroup whose later units are
all invalid (the library takes no single-pulse context, so two and five rows), an odd row count,
pairs that straddle CPIs and rows, sub-block 0 on a workgroup's second unit, and each kernel
instance (0x4433, 0x4402, generic, single-segment).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIR, MF = 0, 1     # rsp_seg_kind
ROWS = (1, 2, 4)
GUARD = 0xA5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _v2(R):
    def build(P):
        from rsp import presets
        return presets.v2(P, R)
    return build


def _dmx(R):
    def build(P):
        from rsp import presets
        return presets.dmx(P, R)
    return build


def _mf_gaps(P):
    """One 4096-point matched filter, nothing else: output columns [0, 10) and [3510, 3600) are
    covered by no segment, and the single-segment launch's rows carry the zero fill."""
    from rsp import presets
    segs = [presets.Segment(MF, 5, 3900, 10, 3500, presets.dmx_replica(), nfft=4096)]
    return presets.Spec("geom", P, 4000, 3600, segs, cfar_segments=[(0, 3600)], radar=presets.radar_params(P, 4000))


def _pc(torch, eng, d_in, batch):
    """pc_dev into CPIs [1, batch] of a [batch + 2] buffer: NaN inside, sentinel bytes in the
    guards.  Returns the inner CPIs as uint32 words."""
    P, W = eng.spec.P, eng.spec.pc_width or eng.spec.R_out
    buf = torch.empty((batch + 2, P, W, 2), dtype=torch.float32, device="cuda")
    buf.view(torch.uint8).fill_(GUARD)
    buf[1:batch + 1] = float("nan")
    eng.pc_dev(d_in, torch.view_as_complex(buf)[1:batch + 1])
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[0].view(np.uint8) == GUARD).all() and (h[-1].view(np.uint8) == GUARD).all(), "a guard CPI was written"
    return np.ascontiguousarray(h[1:-1]).view(np.uint32)


# (id, spec builder, P, batch, fp16 input, fused gain, prune, the pruned instance expected)
CASES = [
    # the fewest rows a context takes (rsp_create wants P >= 2): at rows 4 half the workgroup's
    # units are invalid; five rows: the last workgroup has one valid unit, then only invalid ones
    ("v2-4096-P2", _v2(4096), 2, 1, False, False, 1, 0x4433),
    ("v2-4096-P5", _v2(4096), 5, 1, False, False, 1, 0x4433),
    # three rows: the last workgroup half valid (rows 2), three quarters (rows 4)
    ("v2-4096-P3", _v2(4096), 3, 1, False, False, 1, 0x4433),
    # six rows over two CPIs: at rows 4 a workgroup straddles the CPIs
    ("v2-4096-P3-b2", _v2(4096), 3, 2, False, False, 1, 0x4433),
    # three overlap-save blocks per row, 9 units: pairs straddle rows, sub-block 0 is a second unit
    ("v2-8192-P3", _v2(8192), 3, 1, False, False, 1, 0x4402),
    # five blocks per row, ten units, fp16 input
    ("v2-16384-P2-f16", _v2(16384), 2, 1, True, False, 1, 0x4402),
    ("v2-4096-P3-b2-gain", _v2(4096), 3, 2, False, True, 1, 0x4433),
    ("v2-8192-P3-gain-f16", _v2(8192), 3, 1, True, True, 1, 0x4402),
    # the generic instance of the pair
    ("v2-8192-P3-generic", _v2(8192), 3, 1, False, False, 0, 0),
    # single-segment launches: the zero fill on every unit of the loop; the DMX whole row
    ("mf-4096-gaps-P3", _mf_gaps, 3, 2, False, False, 1, 0),
    ("dmx-4096-P3", _dmx(4096), 3, 1, False, False, 1, 0),
]


@pytest.mark.parametrize("cid,build,P,batch,half,gain,prune,instance", CASES, ids=[c[0] for c in CASES])
def test_rows_bit_identical(torch_cuda, cid, build, P, batch, half, gain, prune, instance):
    from rsp import synth
    from rsp.engine import Engine
    torch = torch_cuda
    spec = build(P)
    echo = synth.echo_numpy(spec, batch, seed=5150)
    d_in = torch.from_numpy(synth.to_half_iq(echo) if half else echo).cuda()
    with Engine(spec, device=0) as eng:
        eng.set_pc_prune(prune)
        if gain:
            eng.set_prefilter(gain=np.linspace(0.5, 2.0, spec.R).astype(np.float32), mti_lag=0)
        plan = eng.pc_plan()
        assert plan["specialised"] == 1 and plan["prune"] == instance
        assert any(s[0] == 4096 for s in plan["segs"])
        out = {}
        for n in ROWS:
            eng.set_pc_rows(n)
            assert eng.pc_rows() == n
            assert eng.pc_plan() == plan   # the plan does not depend on the rows
            out[n] = _pc(torch, eng, d_in, batch)
        eng.set_pc_rows(0)
        assert eng.pc_rows() in ROWS
    one = out[1].view(np.float32)
    assert np.isfinite(one).all(), "unwritten or non-finite output"
    assert np.abs(one).max() > 0
    if cid.startswith("mf-4096-gaps"):
        z = np.ascontiguousarray(out[1].reshape(batch, P, -1, 2))
        assert not z[:, :, :10].any() and not z[:, :, 3510:].any(), "uncovered columns are not +0"
    for n in (2, 4):
        assert np.array_equal(out[n], out[1]), (n, int((out[n] != out[1]).sum()))


def test_chain_rows(torch_cuda):
    """The chain at 128 pulses x 4096 range bins, 3 CPIs, with CFAR: RDM, flag and flagV."""
    from rsp import presets, synth
    from rsp.engine import Engine
    torch = torch_cuda
    P, R, B = 128, 4096, 3
    spec = presets.v2(P, R)
    d_in = torch.from_numpy(synth.echo_numpy(spec, B, seed=5151)).cuda()
    d_other = torch.from_numpy(synth.echo_numpy(spec, B, seed=5153)).cuda()
    out = {}
    with Engine(spec, device=0) as eng:
        cf = presets.default_cfar(spec)

        def run(d_echo):
            d_rdm = torch.full((B, P, R), float("nan"), dtype=torch.float32, device="cuda")
            d_flag = torch.full((B, P, R), 0xFF, dtype=torch.uint8, device="cuda")
            d_fv = torch.full((B, P, R), 0xFF, dtype=torch.uint8, device="cuda")
            eng.run_dev(d_echo, rdm=d_rdm, flag=d_flag, flagV=d_fv, cfar=cf)
            return d_rdm, d_flag, d_fv

        for n in ROWS:
            # the context's PC scratch keeps the previous call's rows: fill it from another echo
            # first (one row per workgroup), so a row this run fails to store cannot pass as written
            eng.set_pc_rows(1)
            run(d_other)
            eng.set_pc_rows(n)
            assert eng.pc_rows() == n
            d_rdm, d_flag, d_fv = run(d_in)
            torch.cuda.synchronize()
            out[n] = (d_rdm.cpu().numpy().view(np.uint32), d_flag.cpu().numpy(), d_fv.cpu().numpy())
    assert np.isfinite(out[1][0].view(np.float32)).all() and out[1][0].view(np.float32).max() > 0
    assert out[1][2].any() and out[1][1].max() <= 1 and out[1][2].max() <= 1
    for n in (2, 4):
        for name, a, b in zip(("rdm", "flag", "flagV"), out[n], out[1]):
            assert np.array_equal(a, b), (n, name, int((a != b).sum()))


def test_other_lengths_keep_one_row(torch_cuda):
    """v2 at 1024 range bins runs the 1024/1024 pair: no multi-row path, whatever is asked for."""
    from rsp import presets, synth
    from rsp.engine import Engine
    torch = torch_cuda
    spec = presets.v2(5, 1024)
    d_in = torch.from_numpy(synth.echo_numpy(spec, 1, seed=5152)).cuda()
    with Engine(spec, device=0) as eng:
        got = []
        for n in ROWS:
            eng.set_pc_rows(n)
            assert eng.pc_rows() == 1
            got.append(_pc(torch, eng, d_in, 1))
    assert np.isfinite(got[0].view(np.float32)).all()
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


def test_arguments(torch_cuda):
    from rsp import RspError, _capi as capi, presets
    from rsp.engine import Engine
    with Engine(presets.v2(4, 4096), device=0) as eng:
        for bad in (-1, 3, 5, 8):
            with pytest.raises(RspError) as ei:
                eng.set_pc_rows(bad)
            assert ei.value.code == capi.RSP_ERR_ARG
        eng.set_pc_rows(2)
        assert eng.pc_rows() == 2
    # a context on the generic PC path has nothing to select (as in test_gpu_pc_prune.py): a
    # 2000-point FIR segment that the 512-point slot of the first matched filter cannot stage
    P, R = 64, 4096
    rp = presets.radar_params(P, R, None)
    pulse2 = presets.lfm(rp["tao"][1], rp["fs"], rp["B"], -1.0)
    pulse3 = presets.lfm(rp["tao"][2], rp["fs"], rp["B"], +1.0)
    spec = presets.lss_spec("v2", P, R, 2000, 300, 1000, pulse2, pulse3,
                            fir_shift=presets.fir_group_delay(presets.FIR_TAPS), radar=rp)
    with Engine(spec, device=0) as eng:
        for n in (0, 1, 2, 4):
            with pytest.raises(RspError) as ei:
                eng.set_pc_rows(n)
            assert ei.value.code == capi.RSP_ERR_UNSUPPORTED
        assert eng.pc_rows() == 1
