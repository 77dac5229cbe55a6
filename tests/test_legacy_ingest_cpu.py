"""The legacy two-beam 24-bit PRT records (frameDataRead_A), CPU side: the integer restatement
tests/legacy_ingest_ref.py pinned by cases worked out by hand from the .m text, the C ABI's
declarations, struct layout and refusals, the file mirror's byte read, and the golden file.
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import legacy_ingest_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "legacy_ingest_3x20.npz")


def _lib():
    from rsp import _capi
    return _capi, _capi.load_library()


# ---------------------------------------------------------------- the restatement, by hand
def test_one_group_by_hand():
    """dataTemp(1:12) = [Ql1 Il1 Qr1 Ir1 Ql2 Il2 Qr2 Ir2 Ql3 Il3 Qr3 Ir3] (1 = high, :85-98)."""
    g = [0x01, 0x12, 0xFF, 0x80,
         0x02, 0x34, 0xFF, 0x00,
         0x03, 0x56, 0xFE, 0x01]
    il, ql, ir, qr = ref.decode_group_bytes(g)
    assert int(ql[0]) == 0x010203 == 66051
    assert int(il[0]) == 0x123456 == 1193046
    assert int(qr[0]) == 0xFFFFFE - 2 ** 24 == -2
    assert int(ir[0]) == 0x800001 - 2 ** 24 == -8388607


def test_sign_rule_is_greater_than():
    assert ref.sign24([0x800000, 0x800001, 0x7FFFFF, 0xFFFFFF, 0, 1]).tolist() == [8388608, -8388607, 8388607, -1, 0, 1]
    assert ref.sign24(ref.EDGE_VALUES).tolist() == list(ref.EDGE_DECODED)


def test_head_by_hand():
    rec = np.zeros(28, dtype=np.uint8)
    rec[0:4] = [0xA5, 0xA5, 0xA5, 0xA5]
    rec[4:8] = [0x34, 0x12, 0x78, 0x56]          # uint16 0x1234 then 0x5678, little-endian
    rec[8:10] = [0x09, 0x00]                     # modFlag 9
    rec[10], rec[11] = 7, 2                      # beamPosNum, beamNums
    rec[12:14] = [0x0B, 0x01]                    # freInd 0x010B
    rec[14:16] = [0xFF, 0x0F]                    # prtInd 4095
    rec[16:26] = 0xEE                            # skipped
    rec[26], rec[27] = 0x12, 0x34
    h, angle = ref.parse_head(rec)
    assert h["frameInd"] == 0x1234 * 65536 + 0x5678 == 305419896
    assert (h["modFlag"], h["beamPosNum"], h["beamNums"], h["freInd"], h["prtInd"], h["sync_ok"]) == (9, 7, 2, 267, 4095, 1)
    assert angle == (18 + 52 * 128) * 360 / 16384 == 146.6455078125          # 2^7, not 2^8
    rec[2] = 0xA4
    assert ref.parse_head(rec)[0]["sync_ok"] == 0


def test_record_size_and_file_names(tmp_path):
    from rsp import ingest
    assert ref.record_bytes(1031) == 12408 == ingest.legacy_record_bytes(1031)
    assert ref.record_bytes(566) == 6828 == ingest.legacy_record_bytes(566)
    for frame, want in ((0, 1), (1, 1), (10, 1), (11, 2), (20, 2), (21, 3)):
        assert ref.file_index(frame) == want == ingest.legacy_file_index(frame), frame
    for ind, want in ((9, "000009.bin"), (10, "000010.bin"), (99, "000099.bin"), (100, "000100.bin")):
        assert os.path.basename(ref.dataFullPathGen("d", ind)) == want
        assert ingest.dataFullPathGen("d", ind) == os.path.join("d", want)
    assert [ingest.legacy_frame_skip(f) for f in (0, 1, 2, 10, 11, 25)] == [-1, 0, 1, 9, 0, 4]


def test_synth_stream_is_what_the_tests_need():
    prt, point = 6, 9
    s = ref.synth_legacy_stream(prt, point, 2, seed=3)
    rec = ref.record_bytes(point)
    assert s.dtype == np.uint8 and s.size == 2 * prt * rec
    d = ref.decode_stream(s, prt, point, 2)
    assert d["status"].tolist() == [0] * (2 * prt) + [2 * prt]
    for z in (d["left"], d["right"]):
        assert z[0, 1, :6].real.tolist() == list(ref.EDGE_DECODED) == z[0, 1, :6].imag.tolist()
    head = d["head"].reshape(2 * prt, 8)
    for k in range(6):
        assert len(set(head[:, k].tolist())) == 2 * prt, ref.HEAD_FIELDS[k]
    assert head[:, 0].max() >= 2 ** 31 and np.all(head[:, 0] % 65536 != head[:, 0] // 65536)
    assert sorted(set(head[:, 6].tolist())) == [0, 1] and not head[:, 7].any()
    raw = s.reshape(2 * prt, rec)
    assert raw[:, 26].min() >= 0x80 and raw[:, 27].min() >= 0x80
    # round trip of the packer through the restatement on all four channels
    rng = np.random.default_rng(1)
    ch = rng.integers(0, 1 << 24, size=(4, 5))
    r = ref.pack_record(ch[0], ch[1], ch[2], ch[3], 1, 2, 3, 4, 5, 6, (0x80, 0x81))
    got = ref.decode_group_bytes(r[28:28 + 60])
    for k in range(4):
        assert got[k].tolist() == ref.sign24(ch[k]).tolist()


def test_truncation_in_the_restatement():
    prt, point = 4, 5
    rec = ref.record_bytes(point)
    s = ref.synth_legacy_stream(prt, point, 1, seed=4)
    whole = ref.decode_stream(s, prt, point)
    for cut, want in ((2 * rec + 10, [0, 0, 1, 1, 2]), (2 * rec + 28 + 30, [0, 0, 1, 1, 2]), (3 * rec - 3, [0, 0, 2, 1, 3]),
                      (3 * rec - 8, [0, 0, 2, 1, 3]), (3 * rec - 9, [0, 0, 1, 1, 2]), (3 * rec, [0, 0, 0, 1, 3])):
        d = ref.decode_stream(s[:cut], prt, point)
        assert d["status"].tolist() == want, cut
        n = want[-1]
        assert np.array_equal(d["left"][0, :n], whole["left"][0, :n]) and not d["left"][0, n:].any()
        assert np.array_equal(d["angle"][0, :n], whole["angle"][0, :n]) and not d["angle"][0, n:].any()
        assert not d["head"][0, n:].any()


# ---------------------------------------------------------------- the C ABI
def test_header_declares_and_library_exports():
    _capi, lib = _lib()
    text = open(os.path.join(ROOT, "include", "rsp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("rsp_legacy_record_bytes", "rsp_ingest_legacy_dev"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in _capi.EXPORTS
    assert "RSP_LEGACY_HEAD_FIELDS = 8" in text and _capi.RSP_LEGACY_HEAD_FIELDS == 8 == len(ref.HEAD_FIELDS)


def test_params_struct_layout_matches_header():
    _capi, _ = _lib()
    fields = ("prt_num", "point_prt", "nframes", "reserved")
    src = ('#include "rsp.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){'
           'printf("%zu", sizeof(rsp_legacy_ingest_params));\n'
           + "".join('printf(" %%zu", offsetof(rsp_legacy_ingest_params, %s));\n' % f for f in fields)
           + 'printf(" %d %d\\n", RSP_LEGACY_HEAD_FIELDS, RSP_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    want = ([C.sizeof(_capi.rsp_legacy_ingest_params)] + [getattr(_capi.rsp_legacy_ingest_params, f).offset for f in fields]
            + [8, 5])
    assert got == want == [16, 0, 4, 8, 12, 8, 5]


def test_record_bytes_export():
    _capi, lib = _lib()
    from rsp.ingest import LegacyIngest
    n = C.c_int64(-1)
    for point in (1, 566, 1031):
        assert lib.rsp_legacy_record_bytes(C.byref(LegacyIngest.params(1536, point, 1)), C.byref(n)) == _capi.RSP_OK
        assert n.value == ref.record_bytes(point) and n.value % 4 == 0
    assert lib.rsp_legacy_record_bytes(None, C.byref(n)) == _capi.RSP_ERR_ARG
    assert lib.rsp_legacy_record_bytes(C.byref(LegacyIngest.params(1536, 1031, 1)), None) == _capi.RSP_ERR_ARG
    assert lib.rsp_legacy_record_bytes(C.byref(LegacyIngest.params(1536, 0, 1)), C.byref(n)) == _capi.RSP_ERR_ARG


def test_null_and_malformed_arguments():
    """Everything is refused before the context is looked at: no GPU needed (ctx == NULL; the
    pointers are never dereferenced)."""
    _capi, lib = _lib()
    from rsp.ingest import LegacyIngest
    P, R, F = 4, 10, 3
    plane = P * R
    stream, out, angle, head, status = 0x10000, 0x200000, 0x300000, 0x400000, 0x500000
    nbytes = F * P * ref.record_bytes(R)

    def dev(p=None, stream=stream, nbytes=nbytes, out=out, bs=0, fs=0, angle=angle, head=head, status=status, **kw):
        if p is None:
            p = LegacyIngest.params(kw.get("P", P), kw.get("R", R), kw.get("F", F))
            p.reserved = kw.get("reserved", 0)
        return lib.rsp_ingest_legacy_dev(None, stream, nbytes, C.byref(p) if p is not False else None, out, bs, fs, angle,
                                         head, status, None)

    def msg():
        return lib.rsp_last_error(None).decode()

    # a well-formed call gets as far as the null context; angle and head may be null
    assert dev() == _capi.RSP_ERR_ARG and "null ctx" in msg()
    assert dev(angle=None, head=None) == _capi.RSP_ERR_ARG and "null ctx" in msg()
    assert dev(nbytes=0) == _capi.RSP_ERR_ARG and "null ctx" in msg()
    for kw in (dict(stream=None), dict(out=None), dict(status=None)):
        assert dev(**kw) == _capi.RSP_ERR_ARG and "null argument" in msg(), kw
    assert dev(p=False) == _capi.RSP_ERR_ARG and "null params" in msg()
    for kw in (dict(P=0), dict(P=-1), dict(R=0), dict(F=0), dict(F=-2), dict(reserved=1), dict(P=65536), dict(F=65536),
               dict(R=(1 << 24) + 1)):
        assert dev(**kw) == _capi.RSP_ERR_ARG and "bad shape" in msg(), kw
    assert dev(nbytes=-1) == _capi.RSP_ERR_ARG and "negative" in msg()
    # strides: the dense ones, both layouts, padded; overlapping planes never
    assert dev(bs=plane, fs=2 * plane) == _capi.RSP_ERR_ARG and "null ctx" in msg()
    assert dev(bs=plane + 3, fs=2 * plane + 9) == _capi.RSP_ERR_ARG and "null ctx" in msg()
    assert dev(bs=F * plane, fs=plane) == _capi.RSP_ERR_ARG and "null ctx" in msg()
    assert dev(bs=(F - 1) * (plane + 5) + plane, fs=plane + 5) == _capi.RSP_ERR_ARG and "null ctx" in msg()
    assert dev(bs=plane - 1, F=1) == _capi.RSP_ERR_ARG and "overlap" in msg()
    assert dev(bs=plane, F=1) == _capi.RSP_ERR_ARG and "null ctx" in msg()
    for bs, fs in ((plane - 1, 0), (plane, 2 * plane - 1), (plane, plane), (F * plane - 1, plane), (F * plane, plane - 1),
                   (-plane, 4 * plane), (plane, -2 * plane), (0, plane)):
        assert dev(bs=bs, fs=fs) == _capi.RSP_ERR_ARG and "overlap" in msg(), (bs, fs)
    # alignment: the stream is read as dwords
    for off in (1, 2, 3):
        assert dev(stream=stream + off) == _capi.RSP_ERR_ARG and "4-byte aligned" in msg()
    assert dev(stream=stream + 4) == _capi.RSP_ERR_ARG and "null ctx" in msg()
    for kw in (dict(out=out + 4), dict(angle=angle + 4), dict(head=head + 2), dict(status=status + 1)):
        assert dev(**kw) == _capi.RSP_ERR_ARG and "misaligned" in msg(), kw


# ---------------------------------------------------------------- the file mirror
def _two_frame_file(tmp_path, prt, point, seed=11):
    s = ref.synth_legacy_stream(prt, point, 2, seed=seed)
    with open(os.path.join(tmp_path, "000001.bin"), "wb") as f:
        f.write(s.tobytes())
    return s


def test_file_mirror_hands_the_right_bytes(tmp_path):
    from rsp import ingest
    prt, point = 3, 7
    s = _two_frame_file(str(tmp_path), prt, point)
    n = prt * ref.record_bytes(point)
    first, second = s[:n].tobytes(), s[n:].tobytes()
    d = str(tmp_path)
    # frameDataRead_A_xzr.m: no seek, the file's first frame whatever frameRInd
    for frame in (0, 1, 2, 10):
        assert ingest.legacy_frame_bytes(d, frame, prt, point) == first == ref.frame_bytes(d, frame, prt, point)
    # Show_Read.m: the seek; frameRInd = 0 gives a negative offset, which does not move
    assert ingest.legacy_frame_bytes(d, 1, prt, point, frame_seek=True) == first
    assert ingest.legacy_frame_bytes(d, 2, prt, point, frame_seek=True) == second == ref.frame_bytes(d, 2, prt, point, True)
    assert ingest.legacy_frame_bytes(d, 0, prt, point, frame_seek=True) == first == ref.frame_bytes(d, 0, prt, point, True)
    assert ingest.legacy_frame_bytes(d, 3, prt, point, frame_seek=True) == b""        # past the file's end
    with pytest.raises(OSError):
        ingest.legacy_frame_bytes(d, 11, prt, point)                                  # 000002.bin is not there
    # the restatement's reader on the same file
    got = ref.frameDataRead_A(d, 2, prt, point, frame_seek=True)
    want = ref.decode_stream(s[n:], prt, point)
    assert np.array_equal(got[0], want["left"][0]) and np.array_equal(got[7], want["angle"][0])
    assert got[2:7] == tuple(int(v) for v in want["head"][0, -1, :5])


# ---------------------------------------------------------------- the golden file
def test_golden_file_matches_the_restatement():
    assert os.path.getsize(GOLDEN) < 8192
    g = np.load(GOLDEN)
    assert sorted(g.files) == ["angle", "head", "left", "right", "stream"]
    prt, point = 3, 20
    assert g["stream"].dtype == np.uint8 and g["stream"].size == prt * ref.record_bytes(point)
    assert np.array_equal(g["stream"], ref.synth_legacy_stream(prt, point, 1, seed=2409))
    d = ref.decode_stream(g["stream"], prt, point)
    for k in ("left", "right", "angle", "head"):
        assert np.array_equal(g[k], d[k][0]), k
    assert g["left"][1, :6].real.tolist() == list(ref.EDGE_DECODED)
