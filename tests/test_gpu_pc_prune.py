"""Pruned pulse-compression instances (rsp_set_pc_prune) against the generic ones.

A pruned instance skips the loads, stores and butterfly operations of whole 1/16-transform
slices that are zero padding (input) or cut by out_len (output).  Every kept operation keeps its
operands and order, so the outputs must be equal value for value: compared with `==`
(np.array_equal), which lets only the sign of an exact zero differ -- the one permitted
difference.  RDM and flags are compared the same way.
"""
import numpy as np
import pytest

import rsp_ref as ref
from _util import RDM_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


# The chain runs at 64 pulses: the default CFAR's Doppler window (2 * (5 + 7) cells beside the
# zero-velocity band) does not fit fewer, and the PC instance depends on R alone.
CHAIN_P = 64


def _run(torch, P, R, batch, prune, half=False, gain=False, seed=4242, chain=True):
    """PC rows of v2 (P, R) through rsp_pc_dev, and RDM, flag, flagV of v2 (CHAIN_P, R) through
    the chain, with the pruned instances on or off."""
    from rsp import presets, synth
    from rsp.engine import Engine

    def engine(p):
        eng = Engine(presets.v2(p, R), device=0)
        eng.set_pc_prune(prune)
        if gain:
            eng.set_prefilter(gain=np.linspace(0.5, 2.0, R).astype(np.float32), mti_lag=0)
        return eng

    def dev(spec, n):
        echo = synth.echo_numpy(spec, n, seed=seed)
        return echo, torch.from_numpy(synth.to_half_iq(echo) if half else echo).cuda()

    with engine(P) as eng:
        echo, d_in = dev(eng.spec, batch)
        d_pc = torch.empty((batch, P, R), dtype=torch.complex64, device="cuda")
        eng.pc_dev(d_in, d_pc)
        torch.cuda.synchronize()
        out = [d_pc.cpu().numpy()]
    if chain:
        with engine(CHAIN_P) as eng:
            _, d_in = dev(eng.spec, 2)
            shp = (2, CHAIN_P, R)
            d_rdm = torch.empty(shp, dtype=torch.float32, device="cuda")
            d_flag = torch.empty(shp, dtype=torch.uint8, device="cuda")
            d_fv = torch.empty(shp, dtype=torch.uint8, device="cuda")
            eng.run_dev(d_in, rdm=d_rdm, flag=d_flag, flagV=d_fv, cfar=presets.default_cfar(eng.spec))
            torch.cuda.synchronize()
            out += [d_rdm.cpu().numpy(), d_flag.cpu().numpy(), d_fv.cpu().numpy()]
    return echo, out


# (P, R, batch, half, gain):
#  4096: the fused 1024/4096 pair, 723 of 1024 and 3145 of 4096 points (slice 12 of the long
#        row partly filled: 12 * 256 = 3072 < 3145 < 3328)
#  8192: overlap-save blocks of 4096, three per row, the last one short (7241 = 2 * 3397 + 447)
# 16384: five blocks per row, fp16 input
@pytest.mark.parametrize("P,R,batch,half,gain", [
    (4, 4096, 3, False, False),
    (4, 4096, 3, False, True),
    (2, 8192, 2, False, False),
    (2, 16384, 2, True, False),
    (2, 16384, 2, True, True),
])
def test_prune_matches_generic(torch_cuda, P, R, batch, half, gain):
    _, on = _run(torch_cuda, P, R, batch, 1, half, gain)
    _, off = _run(torch_cuda, P, R, batch, 0, half, gain)
    assert len(on) == 4
    for name, a, b in zip(("pc", "rdm", "flag", "flagV"), on, off):
        assert np.isfinite(a.view(np.float32) if name == "pc" else a).all(), name
        assert np.array_equal(a, b), (name, int((a != b).sum()))
    assert np.abs(on[0]).max() > 0 and on[1].max() > 0 and on[3].any()


def test_generic_fallback_against_oracle(torch_cuda):
    """v2 at 1024 range bins has no pruned instance (its second segment fills 73 of 1024 points):
    prune on runs the generic kernel, checked against the fp64 oracle at the parity bar."""
    P, R = 16, 1024
    echo, on = _run(torch_cuda, P, R, 2, 1, chain=False)
    _, off = _run(torch_cuda, P, R, 2, 0, chain=False)
    assert on[0].tobytes() == off[0].tobytes()   # the same instance: bytes, not only values
    rp = ref.v2_params(P, R)
    _, p2, p3 = ref.v2_pulses(rp)
    e64 = echo.astype(np.complex128)
    for b in range(2):
        want = ref.fun_lss_pulse_compression(e64[b], p2, p3, 228, 723, R - 951, fir_shift=True)
        err = np.linalg.norm(on[0][b] - want) / np.linalg.norm(want)
        assert err < RDM_TOL, (b, err)


def test_unsupported_on_generic_path(torch_cuda):
    """A context on the generic PC path has nothing to select: here a 2000-point FIR segment
    that the 512-point slot of the first matched filter cannot stage."""
    from rsp import RspError, _capi as capi, presets
    from rsp.engine import Engine
    P, R = 64, 4096
    rp = presets.radar_params(P, R, None)
    pulse2 = presets.lfm(rp["tao"][1], rp["fs"], rp["B"], -1.0)
    pulse3 = presets.lfm(rp["tao"][2], rp["fs"], rp["B"], +1.0)
    spec = presets.lss_spec("v2", P, R, 2000, 300, 1000, pulse2, pulse3,
                            fir_shift=presets.fir_group_delay(presets.FIR_TAPS), radar=rp)
    with Engine(spec, device=0) as eng:
        for enable in (0, 1):
            with pytest.raises(RspError) as ei:
                eng.set_pc_prune(enable)
            assert ei.value.code == capi.RSP_ERR_UNSUPPORTED
        with pytest.raises(RspError) as ei:   # the contract it shares
            eng.set_pc_split(1)
        assert ei.value.code == capi.RSP_ERR_UNSUPPORTED
