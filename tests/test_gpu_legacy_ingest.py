"""GPU decode of the legacy two-beam 24-bit PRT records (rsp_ingest_legacy_dev through
rsp.ingest.LegacyIngest) against the integer restatement of frameDataRead_A_xzr.m
(tests/legacy_ingest_ref.py).

Every comparison is bit-exact: the samples are integers of magnitude <= 2^23 (exact in fp32), the
angles integers * 360 / 2^14 (exact in fp64), heads and status codes integers.
"""
import os

import numpy as np
import pytest

import legacy_ingest_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "legacy_ingest_3x20.npz")


@pytest.fixture(scope="module")
def ing():
    import torch
    assert torch.cuda.is_available()
    from rsp import ingest
    g = ingest.LegacyIngest(0)
    yield g
    g.close()


def _head(h):
    """int32 head columns as the restatement's int64 (frameInd is the unsigned 32-bit pattern)."""
    h = h.astype(np.int64)
    h[..., 0] &= 0xffffffff
    return h


def _check(ing, stream, prt, point, nframes=1, nbytes=None):
    """Decode `stream` (cut to nbytes on the device too) and compare everything with the restatement."""
    nbytes = stream.size if nbytes is None else nbytes
    want = ref.decode_stream(stream[:nbytes], prt, point, nframes)
    out, angle, head, status = ing.decode_dev(ing.upload(stream[:nbytes].tobytes()), nbytes, prt, point, nframes)
    assert out.shape == (nframes, 2, prt, point) and angle.shape == (nframes, prt) and head.shape == (nframes, prt, 8)
    got = out.cpu().numpy()
    assert got.dtype == np.complex64
    assert np.array_equal(got[:, 0].astype(np.complex128), want["left"])
    assert np.array_equal(got[:, 1].astype(np.complex128), want["right"])
    assert np.array_equal(angle.cpu().numpy(), want["angle"])
    assert np.array_equal(_head(head.cpu().numpy()), want["head"])
    assert np.array_equal(status.cpu().numpy(), want["status"])
    return got, want


def test_golden(ing):
    g = np.load(GOLDEN)
    prt, point = g["left"].shape
    out, angle, head, status = ing.decode_dev(ing.upload(g["stream"].tobytes()), g["stream"].size, prt, point)
    got = out.cpu().numpy()
    assert np.array_equal(got[0, 0].astype(np.complex128), g["left"])
    assert np.array_equal(got[0, 1].astype(np.complex128), g["right"])
    assert np.array_equal(angle.cpu().numpy()[0], g["angle"])
    assert np.array_equal(_head(head.cpu().numpy())[0], g["head"])
    assert status.cpu().numpy().tolist() == [0] * prt + [prt]
    assert ing.record_bytes(point) == ref.record_bytes(point) and ing.record_bytes() == 12408


@pytest.mark.parametrize("prt,point", [(3, 1), (2, 63), (2, 64), (3, 65), (5, 257), (4, 1031)])
def test_shapes(ing, prt, point):
    """One sample; both sides of a wave (63, 64, 65); past a 256-thread block (257); the real odd
    width, whose rows are 8-byte aligned only (1031)."""
    _check(ing, ref.synth_legacy_stream(prt, point, 1, seed=100 + point), prt, point)


def test_full_frame(ing):
    prt, point = 1536, 1031
    got, want = _check(ing, ref.synth_legacy_stream(prt, point, 1, seed=5), prt, point)
    assert want["status"][prt] == prt


def test_planted_edge_values(ing):
    """0, 1, 0xFFFFFF, 0x7FFFFF, 0x800000, 0x800001 in every channel: 0x800000 stays +8388608."""
    prt, point = 3, 12
    got, _ = _check(ing, ref.synth_legacy_stream(prt, point, 1, seed=6), prt, point)
    for b in range(2):
        assert got[0, b, 1, :6].real.tolist() == [0.0, 1.0, -1.0, 8388607.0, 8388608.0, -8388607.0]
        assert got[0, b, 1, :6].imag.tolist() == [0.0, 1.0, -1.0, 8388607.0, 8388608.0, -8388607.0]


@pytest.mark.parametrize("layout", ["frame_major", "beam_major"])
def test_strided_output_leaves_the_rest_alone(ing, layout):
    import torch
    prt, point, F = 4, 100, 3
    plane = prt * point
    stream = ref.synth_legacy_stream(prt, point, F, seed=8)
    want = ref.decode_stream(stream, prt, point, F)
    lead = 5
    if layout == "frame_major":
        bs, fs = plane + 3, 2 * plane + 3 + 11
    else:
        fs = plane + 7
        bs = (F - 1) * fs + plane + 13
    total = lead + (F - 1) * fs + bs + plane + 9
    sentinel = np.full(total, np.complex64(complex(-12345.5, 54321.25)))
    buf = torch.from_numpy(sentinel.copy()).to(ing.device)
    out, angle, head, status = ing.decode_dev(ing.upload(stream.tobytes()), stream.size, prt, point, F, out=buf[lead:],
                                              layout=layout, beam_stride=bs, frame_stride=fs)
    got = buf.cpu().numpy()
    touched = np.zeros(total, dtype=bool)
    for f in range(F):
        for b, key in enumerate(("left", "right")):
            o = lead + f * fs + b * bs
            assert not touched[o:o + plane].any()
            touched[o:o + plane] = True
            assert np.array_equal(got[o:o + plane].astype(np.complex128), want[key][f].ravel()), (f, key)
    assert np.array_equal(got[~touched].view(np.uint32), sentinel[~touched].view(np.uint32))
    assert np.array_equal(status.cpu().numpy(), want["status"])
    assert np.array_equal(angle.cpu().numpy(), want["angle"])
    # the dense form of the same layout
    dense = ing.decode_dev(ing.upload(stream.tobytes()), stream.size, prt, point, F, layout=layout)[0].cpu().numpy()
    if layout == "beam_major":
        assert dense.shape == (2, F, prt, point)
        dense = dense.transpose(1, 0, 2, 3)
    assert np.array_equal(dense[:, 0].astype(np.complex128), want["left"])
    assert np.array_equal(dense[:, 1].astype(np.complex128), want["right"])


def test_truncated_streams(ing):
    """A stream cut in the head, in the payload and inside the tail of a middle row (row 4 of 6,
    in the second frame): status codes, decoded-rows count, zero rows and angles from the cut row
    on; the tail-cut row is still decoded."""
    from rsp import _capi
    prt, point, F = 3, 70, 2
    rec = ref.record_bytes(point)
    stream = ref.synth_legacy_stream(prt, point, F, seed=9)
    OK, TR, TT = _capi.RSP_PRT_OK, _capi.RSP_PRT_TRUNCATED, _capi.RSP_PRT_TAIL_TRUNCATED
    for cut, codes, n in ((4 * rec + 13, [OK] * 4 + [TR, TR], 4),                  # head
                          (4 * rec + 28 + 12 * 33 + 5, [OK] * 4 + [TR, TR], 4),    # payload
                          (5 * rec - 9, [OK] * 4 + [TR, TR], 4),                   # one byte short of the payload's end
                          (5 * rec - 8, [OK] * 4 + [TT, TR], 5),                   # the whole tail missing
                          (5 * rec - 3, [OK] * 4 + [TT, TR], 5),                   # inside the tail
                          (5 * rec, [OK] * 5 + [TR], 5),
                          (0, [TR] * 6, 0)):
        got, want = _check(ing, stream, prt, point, F, nbytes=cut)
        assert want["status"].tolist() == codes + [n], cut
        rows = got.reshape(F, 2, prt, point).transpose(0, 2, 1, 3).reshape(F * prt, 2, point)
        assert not rows[n:].any() and all(rows[r].any() for r in range(n))


@pytest.mark.parametrize("frame_seek", [False, True])
def test_frameDataRead_A_from_a_file(ing, tmp_path, frame_seek):
    prt, point = 5, 130
    stream = ref.synth_legacy_stream(prt, point, 2, seed=10)
    with open(os.path.join(str(tmp_path), "000001.bin"), "wb") as f:
        f.write(stream.tobytes())
    got = ing.frameDataRead_A(str(tmp_path), 2, prt, point, frame_seek=frame_seek)
    want = ref.frameDataRead_A(str(tmp_path), 2, prt, point, frame_seek=frame_seek)
    n = prt * ref.record_bytes(point)
    which = ref.decode_stream(stream[n:] if frame_seek else stream[:n], prt, point)
    assert np.array_equal(want[0], which["left"][0])         # the second frame only with the seek
    assert np.array_equal(got[0].cpu().numpy().astype(np.complex128), want[0])
    assert np.array_equal(got[1].cpu().numpy().astype(np.complex128), want[1])
    assert got[2:7] == want[2:7] and got[2] >= 2 ** 31
    assert got[7].dtype == np.float64 and np.array_equal(got[7], want[7])
    # frames of 6 PRTs: the second starts at record 6 of the file's 10, which ends it after 4 rows
    with pytest.raises(ValueError, match="PRT 5 of 6"):
        ing.frameDataRead_A(str(tmp_path), 2, prt + 1, point, frame_seek=True)


def test_dmx_chain_from_records():
    """DmxFrameProcessor.process_records_dev == process_dev fed the restatement's echo, bit for
    bit, on every plane and estimate; the beam position and the frequency number come from each
    frame's last PRT.  P = 1536 with a 2048-point Doppler is the waveform's own slow-time shape
    (the two-beam MTD instance the other suites exercise); R is small."""
    import torch
    from rsp.dmx import DmxFrameProcessor
    P, R, F = 1536, 100, 2
    proc = DmxFrameProcessor(freInd=2, P=P, R=R)
    stream = ref.synth_legacy_stream(P, R, F, seed=12, freInd=2, beamPosNum=(4, 7))
    want = ref.decode_stream(stream, P, R, F)
    d_stream = torch.from_numpy(stream).to(proc.device)
    runs = proc.process_records_dev(d_stream, stream.size, F)
    assert [r["frames"] for r in runs] == [(0, 1), (1, 2)] and [r["beamPosNum"] for r in runs] == [4, 7]
    echo = np.stack([want["left"], want["right"]], axis=1).astype(np.complex64)
    for r, bpn in zip(runs, (4, 7)):
        a, b = r["frames"]
        one = proc.process_dev(torch.from_numpy(echo[a:b]).to(proc.device), bpn)
        torch.cuda.synchronize()
        assert len(one) == 8
        for k, v in one.items():
            if not isinstance(v, tuple):                       # the planes
                assert np.array_equal(v.cpu().numpy().view(np.uint8), r[k].cpu().numpy().view(np.uint8)), k
                continue
            # (est, cells, count): the rows past a CPI's count are not written
            (est, cells, count), (est2, cells2, count2) = ([t.cpu().numpy() for t in x] for x in (v, r[k]))
            assert np.array_equal(count, count2), k
            for c in range(b - a):
                n = min(int(count[c, 0]), est.shape[1])
                assert np.array_equal(est[c, :n].view(np.uint8), est2[c, :n].view(np.uint8)), k
                assert np.array_equal(cells[c, :n], cells2[c, :n]), k
        assert np.array_equal(r["angleCode"], np.fmod(want["angle"][a:b] + 29.01 + 5.9, 360.0))
        assert r["frameInd"].tolist() == want["head"][a:b, -1, 0].tolist()
    # both frames at one beam position: one run
    same = stream.copy().reshape(F * P, ref.record_bytes(R))
    same[:, 10] = 4
    runs = proc.process_records_dev(torch.from_numpy(same.ravel()).to(proc.device), same.size, F)
    assert len(runs) == 1 and runs[0]["frames"] == (0, 2) and runs[0]["sum"].shape[0] == 2
    # a foreign frequency number in the second frame's last PRT
    bad = stream.copy().reshape(F * P, ref.record_bytes(R))
    bad[F * P - 1, 12] = 3
    with pytest.raises(ValueError, match="freInd 3"):
        proc.process_records_dev(torch.from_numpy(bad.ravel()).to(proc.device), bad.size, F)
    with pytest.raises(ValueError, match="ends inside"):
        proc.process_records_dev(d_stream, stream.size - 9, F)
    proc.close()
