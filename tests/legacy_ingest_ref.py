"""Integer restatement of MatlabProcess_xuzerui/frameDataRead_A_xzr.m (the three-argument
frameDataRead_A, :15-150), statement for statement in numpy, with Show_Read.m's in-file frame
seek (:45) as an option.  MATLAB's 1-based strided picks dataTemp(k:12:end) are data[k-1::12].

What the .m text does and a rewrite tends to get wrong:
  * frameInd = frameInd1*2^16 + frameInd2 with the FIRST uint16 the high word (:60-62);
  * angleCode = (angleCode1 + angleCode2*2^7)*360/16384 -- 2^7, not 2^8 (:75-77);
  * the 12-byte group is [Ql Il Qr Ir] high bytes, then middle bytes, then low bytes (:85-98);
  * the sign fix is `> 2^23` (:112-129), so 0x800000 stays +8388608;
  * the seek to the frame is commented out in frameDataRead_A_xzr.m (:48): it always decodes the
    file's first frame; Show_Read.m (:45) seeks, and a negative offset (frameRInd = 0) makes
    fseek fail without moving.

synth_legacy_stream() packs chosen samples and head fields into record bytes for the tests.
"""
import os

import numpy as np

FRAMES_EACH_FILE = 10                                  # :34
HEAD_FIELDS = ("frameInd", "modFlag", "beamPosNum", "beamNums", "freInd", "prtInd", "sync_ok", "zero")
EDGE_VALUES = (0, 1, 0xFFFFFF, 0x7FFFFF, 0x800000, 0x800001)
EDGE_DECODED = (0, 1, -1, 8388607, 8388608, -8388607)


def record_bytes(point_PRT=1031):
    """bytesTotalEachPRT = bytesFrameHead + bytesFrameEnd + 12*point_PRT + 4 (:27-31)."""
    return 24 + 8 + 12 * point_PRT + 4


def file_index(frameRInd):
    """fix((frameRInd-1)/framesEachFile)+1 (:40)."""
    return int(np.fix((frameRInd - 1) / FRAMES_EACH_FILE)) + 1


def dataFullPathGen(DataFilePath, fileInd):
    """dataFullPathGen.m:3-11."""
    if fileInd < 10:
        name = "00000" + str(fileInd) + ".bin"
    elif fileInd < 100:
        name = "0000" + str(fileInd) + ".bin"
    else:
        name = "000" + str(fileInd) + ".bin"
    return os.path.join(DataFilePath, name)


def sign24(v):
    """if v > 2^23, v = v - 2^24 (:112-129), on int64 arrays."""
    v = np.asarray(v, dtype=np.int64)
    return np.where(v > 2 ** 23, v - 2 ** 24, v)


def decode_group_bytes(data):
    """dataTemp (uint8, 12 bytes per sample) -> (I_left, Q_left, I_right, Q_right) int64 (:83-130)."""
    d = np.asarray(data, dtype=np.uint8).astype(np.int64)
    I_left3, Q_left3, I_right3, Q_right3 = d[9::12], d[8::12], d[11::12], d[10::12]      # low bytes   (:85-88)
    I_left2, Q_left2, I_right2, Q_right2 = d[5::12], d[4::12], d[7::12], d[6::12]        # middle      (:90-93)
    I_left1, Q_left1, I_right1, Q_right1 = d[1::12], d[0::12], d[3::12], d[2::12]        # high        (:95-98)
    return (sign24(I_left1 * 2 ** 16 + I_left2 * 2 ** 8 + I_left3), sign24(Q_left1 * 2 ** 16 + Q_left2 * 2 ** 8 + Q_left3),
            sign24(I_right1 * 2 ** 16 + I_right2 * 2 ** 8 + I_right3),
            sign24(Q_right1 * 2 ** 16 + Q_right2 * 2 ** 8 + Q_right3))


def parse_head(rec):
    """The 28 head bytes as the reference's freads take them (:56-77) -> (fields dict, angleCode)."""
    u16 = np.frombuffer(bytes(rec[:16]), dtype="<u2").astype(np.int64)
    frameInd = int(u16[2]) * 2 ** 16 + int(u16[3])
    h = dict(frameInd=frameInd, modFlag=int(u16[4]), beamPosNum=int(rec[10]), beamNums=int(rec[11]),
             freInd=int(u16[6]), prtInd=int(u16[7]), sync_ok=int(u16[0] == 0xA5A5 and u16[1] == 0xA5A5), zero=0)
    angleCode = (int(rec[26]) + int(rec[27]) * 2 ** 7) * 360 / 16384
    return h, angleCode


def decode_stream(stream, prtNum, point_PRT, nframes=1):
    """nframes * prtNum consecutive records -> dict(left, right complex128 [nframes][prtNum][point],
    angle float64 [nframes][prtNum], head int64 [nframes][prtNum][8], status int32 [rows + 1]).
    Status codes as include/rsp.h: 0 whole, 1 head or payload cut (that row and all later ones are
    zeros), 2 only the tail cut (decoded); last entry the rows decoded."""
    buf = np.frombuffer(bytes(stream), dtype=np.uint8)
    rec = record_bytes(point_PRT)
    rows = nframes * prtNum
    left = np.zeros((rows, point_PRT), dtype=np.complex128)
    right = np.zeros((rows, point_PRT), dtype=np.complex128)
    angle = np.zeros(rows, dtype=np.float64)
    head = np.zeros((rows, len(HEAD_FIELDS)), dtype=np.int64)
    status = np.zeros(rows + 1, dtype=np.int32)
    decoded, stopped = 0, False
    for r in range(rows):
        base = r * rec
        if stopped or base + rec - 8 > buf.size:
            status[r] = 1
            stopped = True
            continue
        h, angle[r] = parse_head(buf[base:base + 28])
        head[r] = [h[k] for k in HEAD_FIELDS]
        il, ql, ir, qr = decode_group_bytes(buf[base + 28:base + 28 + 12 * point_PRT])
        left[r] = il + 1j * ql                                                               # :132
        right[r] = ir + 1j * qr                                                              # :133
        status[r] = 0 if base + rec <= buf.size else 2
        decoded += 1
    status[rows] = decoded
    shp = (nframes, prtNum)
    return dict(left=left.reshape(shp + (point_PRT,)), right=right.reshape(shp + (point_PRT,)), angle=angle.reshape(shp),
                head=head.reshape(shp + (len(HEAD_FIELDS),)), status=status)


def frame_bytes(orgDataFilePath, frameRInd, prtNum, point_PRT=1031, frame_seek=False):
    """The bytes the PRT loop reads (:40-53; Show_Read.m:35-49 with frame_seek)."""
    n = record_bytes(point_PRT) * prtNum
    with open(dataFullPathGen(orgDataFilePath, file_index(frameRInd)), "rb") as f:
        frameSkip = int(np.fmod(frameRInd - 1, FRAMES_EACH_FILE))                            # rem (:46)
        if frame_seek and n * frameSkip >= 0:                                               # fseek fails on < 0
            f.seek(n * frameSkip)
        return f.read(n)


def frameDataRead_A(orgDataFilePath, frameRInd, prtNum, point_PRT=1031, frame_seek=False):
    """-> (Left, Right, frameInd, modFlag, beamPosNum, beamNums, freInd, angleCodeSeries); the
    scalars are those of the last PRT read."""
    d = decode_stream(frame_bytes(orgDataFilePath, frameRInd, prtNum, point_PRT, frame_seek), prtNum, point_PRT, 1)
    if d["status"][prtNum] < prtNum:
        raise ValueError("short file")
    h = dict(zip(HEAD_FIELDS, d["head"][0, -1]))
    return (d["left"][0], d["right"][0], int(h["frameInd"]), int(h["modFlag"]), int(h["beamPosNum"]), int(h["beamNums"]),
            int(h["freInd"]), d["angle"][0])


def pack_record(il, ql, ir, qr, frameInd, modFlag, beamPosNum, beamNums, freInd, prtInd, angle_bytes, sync=(0xA5A5, 0xA5A5),
                filler=0):
    """One record from unsigned 24-bit channel values (arrays of point_PRT) and head fields."""
    n = len(il)
    rec = np.full(record_bytes(n), filler, dtype=np.uint8)
    rec[0:16] = np.frombuffer(np.array([sync[0], sync[1], (frameInd >> 16) & 0xffff, frameInd & 0xffff, modFlag,
                                        beamPosNum | (beamNums << 8), freInd, prtInd], dtype="<u2").tobytes(), dtype=np.uint8)
    rec[26], rec[27] = angle_bytes
    g = np.zeros((n, 12), dtype=np.uint8)
    for k, ch in enumerate((ql, il, qr, ir)):                                               # byte order within a part
        ch = np.asarray(ch, dtype=np.int64)
        g[:, k], g[:, 4 + k], g[:, 8 + k] = (ch >> 16) & 0xff, (ch >> 8) & 0xff, ch & 0xff
    rec[28:28 + 12 * n] = g.ravel()
    return rec


def synth_legacy_stream(prt, point, nframes, seed, freInd=None, beamPosNum=None):
    """Record bytes (uint8 array) of nframes * prt PRTs: samples uniform over the full 24-bit range,
    independent per channel (any byte or channel swap shows); row 1 of frame 0 (row 0 when prt is 1)
    starts with EDGE_VALUES in every channel, as far as point allows; every PRT has its own frameInd
    (both 16-bit words used), prtInd, modFlag, beamPosNum, beamNums and freInd; both angle bytes are
    >= 0x80 (so 2^7 and 2^8 differ); every fifth PRT has a wrong sync word; the skipped head bytes
    and the tail are 0xEE.  freInd / beamPosNum, if given, replace the per-PRT values (per frame
    if a sequence)."""
    rng = np.random.default_rng(seed)
    recs = []
    for f in range(nframes):
        for p in range(prt):
            r = f * prt + p
            ch = rng.integers(0, 1 << 24, size=(4, point), dtype=np.int64)
            if r == min(1, prt - 1):
                k = min(point, len(EDGE_VALUES))
                ch[:, :k] = np.asarray(EDGE_VALUES[:k])[None, :]
            ab = (0x80 + int(rng.integers(0, 0x80)), 0x80 + int(rng.integers(0, 0x80)))
            fre = (0x0100 + r) % 0x10000 if freInd is None else int(np.ravel(freInd)[f % np.size(freInd)])
            bpn = (3 + 7 * r) % 256 if beamPosNum is None else int(np.ravel(beamPosNum)[f % np.size(beamPosNum)])
            sync = (0xA5A5, 0xA5A5) if r % 5 != 4 else ((0xA5A4, 0xA5A5) if r % 10 == 4 else (0xA5A5, 0x5A5A))
            recs.append(pack_record(ch[0], ch[1], ch[2], ch[3], frameInd=(0x9ABC0000 + 0x00010003 * r + 7) & 0xffffffff,
                                    modFlag=(0x8001 + 5 * r) & 0xffff, beamPosNum=bpn, beamNums=(200 - r) % 256,
                                    freInd=fre, prtInd=(0xF000 + r) & 0xffff, angle_bytes=ab, sync=sync, filler=0xEE))
    return np.concatenate(recs)
