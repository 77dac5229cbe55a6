"""Per-pipeline chunk sizes (rsp_set_lane_chunks): pipeline i cuts its own chunks of cpis[i] CPIs,
so the batch is cut A, B, A, B, ... and the pipelines' periods differ.  Everything sized per
pipeline -- the PC scratch and concat staging slots, the internal RDM slots, the hit-list slots of
the grouped range stage -- must use the pipeline's fixed capacity, never the current chunk's size.
The chunking only changes which launches overlap, so every output is BIT-identical to the
equal-chunk schedule, v2 64 x 1024 with the default CFAR."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _chain(torch, spec, echo, cfar, chunk=0, lanes=(), streams=0, want_rdm=True):
    from rsp.engine import Engine
    with Engine(spec, device=0, chunk=chunk, streams=streams) as eng:
        if lanes:
            eng.set_lane_chunks(lanes)
        shp = (echo.shape[0], spec.V, spec.R_out)
        rdm = torch.empty(shp, dtype=torch.float32, device="cuda") if want_rdm else None
        flag = torch.empty(shp, dtype=torch.uint8, device="cuda") if cfar else None
        fv = torch.empty(shp, dtype=torch.uint8, device="cuda") if cfar else None
        eng.run_dev(echo, rdm=rdm, flag=flag, flagV=fv, cfar=cfar)
        torch.cuda.synchronize()
        return tuple(None if t is None else t.cpu().numpy() for t in (rdm, flag, fv))


@pytest.fixture(scope="module")
def case(torch_cuda):
    """v2 64 x 1024, 60 CPIs, and the equal-chunk reference (rsp_set_chunk(3), two pipelines) of
    the whole batch and of its first 11 CPIs -- computed once, never modified."""
    from rsp import presets, synth
    spec = presets.v2(64, 1024)
    cfar = presets.default_cfar(spec)
    echo = synth.echo_torch(spec, 60, seed=2311, device="cuda")
    ref60 = _chain(torch_cuda, spec, echo, cfar, chunk=3)
    ref11 = _chain(torch_cuda, spec, echo[:11], cfar, chunk=3)
    assert ref11[1].sum() > 0 and ref60[1].sum() > ref11[1].sum()
    for a, b in zip(ref11, ref60):
        assert np.array_equal(a, b[:11])   # (a CPI's outputs do not depend on the batch around it)
    return spec, cfar, echo, ref11, ref60


def _same(got, want):
    for name, a, b in zip(("rdm", "flag", "flagV"), got, want):
        if a is None:
            continue
        assert a.tobytes() == b.tobytes(), (name, int((a != b).sum()))


@pytest.mark.parametrize("lanes", [(3, 2), (2, 3), (4, 1)])
def test_lane_chunks_bit_exact(torch_cuda, case, lanes):
    """Batch 11: (3, 2) ends 3 2 3 2 1 with the short chunk on pipeline 0, (2, 3) ends 2 3 2 3 1,
    (4, 1) ends 4 1 4 1 1 -- the short chunk where the pipeline's own size is 4."""
    spec, cfar, echo, ref11, _ = case
    _same(_chain(torch_cuda, spec, echo[:11], cfar, lanes=lanes), ref11)


def test_lane_chunks_cross_a_range_group(torch_cuda, case):
    """Batch 60 in chunks of (2, 1): 20 chunks per pipeline, so each crosses a 16-chunk group of
    the grouped range stage, whose hit-list slots and region counts are the pipeline's own."""
    spec, cfar, echo, _, ref60 = case
    _same(_chain(torch_cuda, spec, echo, cfar, lanes=(2, 1)), ref60)


def test_lane_chunks_without_rdm_output(torch_cuda, case):
    """Flags only: the internal RDM slots (sized by the largest chunk) and the fused range stage,
    the fallback where the range stages cannot be grouped."""
    spec, cfar, echo, ref11, _ = case
    got = _chain(torch_cuda, spec, echo[:11], cfar, lanes=(3, 2), want_rdm=False)
    assert got[0] is None
    _same(got, ref11)


def test_lane_chunks_api(torch_cuda, case):
    """() restores the default, a later rsp_set_chunk means equal chunks, bad lists are refused."""
    from rsp import RspError, _capi as capi
    from rsp.engine import Engine
    spec, cfar, echo, ref11, _ = case
    with Engine(spec, device=0) as eng:
        for bad in ((0, 2), (3, -1), (1, 2, 3, 4, 5)):
            with pytest.raises(RspError) as ei:
                eng.set_lane_chunks(bad)
            assert ei.value.code == capi.RSP_ERR_ARG
        eng.set_lane_chunks((4, 1))
        eng.set_lane_chunks(())
        eng.set_lane_chunks((1, 5, 2))
        eng.set_chunk(3)
    _same(_chain(torch_cuda, spec, echo[:11], cfar, lanes=(5, 1, 2)), ref11)   # three pipelines


@pytest.mark.parametrize("chunk,lanes", [(4, ()), (0, (4, 3))])
def test_concat_short_last_chunk_on_second_pipeline(torch_cuda, chunk, lanes):
    """legacy_concat stages full-width PC rows in a per-pipeline slot before the range gather.
    Batch 6 in chunks of 4 (or (4, 3)) on two pipelines puts a short chunk of 2 on pipeline 1: its
    slot must start at the slot capacity, not at 2 CPIs' rows -- inside pipeline 0's slot, which
    pipeline 0 may still be gathering from.  Against the single-pipeline run, bit for bit."""
    torch = torch_cuda
    from rsp import presets, synth
    spec = presets.legacy(96, 1031, concat=True)
    echo = torch.from_numpy(synth.echo_numpy(spec, 6, seed=2320)).cuda()
    want = _chain(torch, spec, echo, None, chunk=4, streams=1)
    assert np.isfinite(want[0]).all() and want[0].max() > 0
    for _ in range(3):   # (a race need not show on the first run)
        _same(_chain(torch, spec, echo, None, chunk=chunk, lanes=lanes, streams=2), want)
