"""The CFAR kernels across their dispatch table, on designed scenes, against the fp64 oracle.

Which kernel a CFAR call runs is decided on the host from the shape, the window, the segments'
presence, the chunk plan and whether the caller passes an RDM buffer ("The CFAR
dispatch table").  Every row of STANDALONE and FUSED is one point chosen to sit on a boundary of
those rules, with the plan it must select written by hand from the rules (rsp_cfar_plan /
Engine.cfar_plan reports what the launchers' own predicates choose; never copied from it).

The input is a scene of tests/cfar_scene.py: Rayleigh noise with spikes on the first and last
cells of every segment and of the Doppler band, on the cells where a window first fits, across
the 4- and 16-cell words of the range kernels, ties, a run that passes the Doppler test only, and
zeros.  Every scene runs at T = 3 (the features decide) and T = 1.5 (noise hits are dense, so
every branch of every thread sees hits).  tests/test_cfar_scene_cpu.py checks the scenes
themselves, without a GPU.

Every output goes into the middle of a buffer of 0xA5 bytes with one CPI plane of guard on either
side: the guards must come back untouched and every inner byte as 0 or 1.  Flags are compared
with the C oracle (oracle_flags_c) fed the very fp32 values the kernels read -- the call's input
for rsp_cfar_dev, the RDM the same call returned for the chain -- so the flag logic is tested
alone: no mismatch outside the oracle's near-threshold mask, at most as many inside it as it has
cells, and the mask itself (outside the scenes' deliberate ties) at most 0.1 % of the cells.
"""
import dataclasses
import functools

import numpy as np
import pytest

import cfar_scene as cs
import rsp_ref as ref
from _util import NEAR_TOL, RDM_TOL, flag_mismatch, oracle_flags_c

MASK_CAP = 1e-3        # of the scene's cells
SENTINEL = 0xA5
W57 = (5, 7, 5, 7)     # refV, saveV, refR, saveR
# rsp_cfar_plan_t codes (include/rsp.h)
COPY, GENERIC, CELL4, CELL16 = range(4)
NONE, GROUPED, JOB57, PREV_HITS, PER_CHUNK = range(5)
H_NONE, H_BATCHED57, H_PER_HIT57, H_RUNTIME = range(4)


def cfar_obj(win, T, M0, zdiv, segs, methods, rflag=1):
    from rsp import presets
    return presets.Cfar(refV=win[0], saveV=win[1], refR=win[2], saveR=win[3], TV=T, TR=T, methodV=methods[0],
                        methodR=methods[1], M0=M0, rFlag=rflag, zero_v_div=zdiv, segments=list(segs))


@functools.lru_cache(maxsize=None)
def scene(V, R, nseg, M0, zdiv, win, mtd_zdiv=0, seed=cs.SEED):
    return cs.build(V, R, cs.layout(R, win[2] + win[3], nseg), M0, zdiv, *win, mtd_zero_div=mtd_zdiv, seed=seed)


def tie_zone(sc):
    """Cells whose outcome an exact tie of the scene decides (the oracle's mask holds them by design)."""
    z = np.zeros(sc.field.shape, bool)
    for f in sc.features:
        if f.tie:
            for v, c, _ in f.cells:
                z[v, max(c - 2, 0):c + 3] = True
    return z


# ------------------------------------------------------------------------------ (a) stand-alone
@dataclasses.dataclass(frozen=True)
class S:
    """rsp_cfar_dev on [2][V][R].  plan = (log2 tile width of cfar_v_kernel, range kernel, its
    workgroups per row).  cfar_v_kernel: the widest tile of 64, 32, ... columns with
    2 * W * (V + 1) * 4 <= 96 KiB -- 64 up to V = 191, 32 up to 383, 16 from 384.  Range kernel:
    rFlag = 0 copies; 5 + 7 with R % 16 == 0 the 16-cell kernel, ceil(R / 16 / 256) workgroups per
    row; 5 + 7 with R % 4 == 0 the 4-cell kernel, ceil(R / 4 / 256); anything else the generic one."""
    id: str
    V: int
    M0: int
    R: int
    nseg: int
    zdiv: int
    methods: tuple
    plan: tuple
    win: tuple = W57
    rflag: int = 1


STANDALONE = [
    # ---- 5 + 7, R % 16 == 0: cfar_r16_kernel; V walks the Doppler tile widths, M0 its two extremes
    S("r16-v25-none", 25, 0, 272, 0, 0, (0, 0), (6, CELL16, 1)),            # band of exactly 24 rows
    S("r16-v27-inner", 27, 1, 272, 1, 20, (0, 1), (6, CELL16, 1)),          # likewise, M0 = 1
    S("r16-v64-four", 64, 0, 272, 4, 20, (1, 0), (6, CELL16, 1)),
    S("r16-v64-m0max-four", 64, 19, 272, 4, 0, (1, 1), (6, CELL16, 1)),     # (63 - 24) // 2
    S("r16-v191-none", 191, 0, 272, 0, 20, (1, 1), (6, CELL16, 1)),
    S("r16-v192-inner", 192, 0, 272, 1, 0, (0, 0), (5, CELL16, 1)),
    S("r16-v383-four", 383, 0, 272, 4, 20, (0, 1), (5, CELL16, 1)),
    S("r16-v384-none", 384, 0, 272, 0, 0, (1, 0), (4, CELL16, 1)),
    S("r16-2wg-four", 25, 0, 4112, 4, 0, (0, 0), (6, CELL16, 2)),           # 257 threads' worth of a row
    S("r16-2wg-none", 25, 0, 4112, 0, 20, (1, 1), (6, CELL16, 2)),
    S("r16-narrow-none", 64, 0, 48, 0, 0, (0, 0), (6, CELL16, 1)),          # one partly filled Doppler tile
    S("r16-narrow-inner", 384, 0, 48, 1, 20, (1, 1), (4, CELL16, 1)),
    # ---- 5 + 7, R % 4 == 0 only: cfar_r_kernel
    S("r4-v25-none", 25, 0, 268, 0, 0, (0, 0), (6, CELL4, 1)),
    S("r4-v64-inner", 64, 0, 268, 1, 20, (0, 1), (6, CELL4, 1)),
    S("r4-v64-four", 64, 0, 268, 4, 20, (1, 0), (6, CELL4, 1)),
    S("r4-v192-m0max-four", 192, 83, 268, 4, 0, (1, 1), (5, CELL4, 1)),     # (191 - 24) // 2
    S("r4-2wg-four", 25, 0, 1028, 4, 0, (0, 1), (6, CELL4, 2)),
    S("r4-2wg-inner", 25, 0, 1028, 1, 20, (1, 0), (6, CELL4, 2)),
    # ---- 5 + 7, R % 4 != 0: cfar_r_generic_kernel
    S("gen-r270-none", 64, 0, 270, 0, 0, (0, 0), (6, GENERIC, 0)),
    S("gen-r270-four", 64, 0, 270, 4, 20, (1, 1), (6, GENERIC, 0)),
    S("gen-r269-inner", 27, 1, 269, 1, 0, (0, 1), (6, GENERIC, 0)),
    S("gen-r269-four", 191, 0, 269, 4, 20, (1, 0), (6, GENERIC, 0)),
    # ---- other windows: the generic kernel whatever R; (16, 14) is the largest it was built for
    S("w5-4-r272-four", 64, 0, 272, 4, 0, (0, 0), (6, GENERIC, 0), (5, 4, 5, 4)),
    S("w5-4-r269-m0max", 25, 3, 269, 0, 20, (1, 1), (6, GENERIC, 0), (5, 4, 5, 4)),   # (24 - 18) // 2
    S("w3-2-r272-inner", 27, 1, 272, 1, 0, (0, 1), (6, GENERIC, 0), (3, 2, 3, 2)),
    S("w3-2-r269-four", 64, 0, 269, 4, 20, (1, 0), (6, GENERIC, 0), (3, 2, 3, 2)),
    S("w8-4-r272-none", 64, 0, 272, 0, 20, (1, 0), (6, GENERIC, 0), (8, 4, 8, 4)),
    S("w8-4-r269-four", 25, 0, 269, 4, 0, (0, 1), (6, GENERIC, 0), (8, 4, 8, 4)),     # band of exactly 2 * 12
    S("w1-0-r272-four", 25, 0, 272, 4, 20, (1, 1), (6, GENERIC, 0), (1, 0, 1, 0)),
    S("w1-0-r269-m0max", 64, 30, 269, 1, 0, (0, 0), (6, GENERIC, 0), (1, 0, 1, 0)),   # 3 rows left
    S("w16-14-r272-four", 64, 0, 272, 4, 0, (0, 1), (6, GENERIC, 0), (16, 14, 16, 14)),
    S("w16-14-r269-four", 64, 1, 269, 4, 20, (1, 0), (6, GENERIC, 0), (16, 14, 16, 14)),   # M0 max: 61 rows
    # ---- rFlag = 0: flag = flagV
    S("copy-r272-four", 64, 0, 272, 4, 20, (0, 0), (6, COPY, 0), rflag=0),
    S("copy-r272-none", 192, 0, 272, 0, 0, (0, 1), (5, COPY, 0), rflag=0),
    S("copy-r269-inner", 27, 1, 269, 1, 0, (1, 0), (6, COPY, 0), rflag=0),
    S("copy-r269-four", 64, 19, 269, 4, 20, (1, 1), (6, COPY, 0), rflag=0),
]
THRESHOLDS = (3.0, 1.5)


def standalone_scenes(case):
    """The two CPIs of a case: the same features on two noise seeds."""
    return [scene(case.V, case.R, case.nseg, case.M0, case.zdiv, case.win, 0, cs.SEED + b) for b in range(2)]


def _guard_bytes(shape, itemsize):
    """One CPI plane, rounded up to 256 bytes so that the inner planes keep the allocation's alignment."""
    plane = int(np.prod(shape[1:])) * itemsize
    return plane, -(-plane // 256) * 256


def guarded(torch, shape, dtype):
    """A buffer of sentinel bytes -- a guard plane, [batch, V, R], a guard plane -- and its inner view."""
    itemsize = torch.empty((), dtype=dtype).element_size()
    plane, g = _guard_bytes(shape, itemsize)
    raw = torch.full((2 * g + shape[0] * plane,), SENTINEL, dtype=torch.uint8, device="cuda")
    return raw, raw[g:g + shape[0] * plane].view(dtype).view(tuple(shape))


def check_guards(raw, shape, itemsize=1):
    plane, g = _guard_bytes(shape, itemsize)
    h = raw.cpu().numpy()
    assert (h[:g] == SENTINEL).all() and (h[g + shape[0] * plane:] == SENTINEL).all(), "a guard plane was written"
    return h[g:g + shape[0] * plane]


def check_flags(got_flag, got_fv, rdm64, cf, scenes, what):
    """The rules of the module docstring; returns (mask cells, soft mismatches) for the record."""
    assert got_flag.max() <= 1 and got_fv.max() <= 1, what + ": a flag byte that is neither 0 nor 1"
    flag, flagV, amb = oracle_flags_c(rdm64, cf, NEAR_TOL)
    hard, soft = flag_mismatch(got_flag, flag, amb)
    hardv, softv = flag_mismatch(got_fv, flagV, amb)
    print("%s: flags %d / %d Doppler hits, mask %d, mismatches hard %d+%d soft %d+%d"
          % (what, int(flag.sum()), int(flagV.sum()), int(amb.sum()), hard, hardv, soft, softv))
    assert hard == 0 and hardv == 0, (what, hard, hardv)
    assert soft <= int(amb.sum()) and softv <= int(amb.sum()), (what, soft, softv)
    ties = np.stack([tie_zone(s) for s in scenes])
    assert (amb & ~ties).sum() <= MASK_CAP * amb.size, (what, int((amb & ~ties).sum()))
    return flag, flagV, amb


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def cfar_engine(torch_cuda):
    from rsp.engine import Engine
    eng = Engine(None, device=0)
    yield eng
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("T", THRESHOLDS)
@pytest.mark.parametrize("case", STANDALONE, ids=lambda c: c.id)
def test_standalone(torch_cuda, cfar_engine, case, T):
    torch = torch_cuda
    eng = cfar_engine
    scenes = standalone_scenes(case)
    segs = scenes[0].segments
    cf = cfar_obj(case.win, T, case.M0, case.zdiv, segs, case.methods, case.rflag)
    lw, kern, groups = case.plan
    assert eng.cfar_plan(cf, 2, V=case.V, R=case.R, fused=False) == dict(fused=0, v_tile_log2=lw, r_kernel=kern,
                                                                      r_groups=groups)
    x = np.stack([s.field for s in scenes]).astype(np.float32)
    assert (x.astype(np.float64) == np.stack([s.field for s in scenes])).all()   # the oracle reads the same values
    d_x = torch.from_numpy(x).cuda()
    shape = x.shape
    raw_f, d_flag = guarded(torch, shape, torch.uint8)
    raw_v, d_fv = guarded(torch, shape, torch.uint8)
    eng.cfar_dev(d_x, d_flag, d_fv, cfar=cf)
    torch.cuda.synchronize()
    got_flag = check_guards(raw_f, shape).reshape(shape)
    got_fv = check_guards(raw_v, shape).reshape(shape)
    flag, flagV, amb = check_flags(got_flag, got_fv, x.astype(np.float64), cf, scenes, case.id)
    # the input is exact, so a tie is decided by the first-maximum rule alone: inside the mask too,
    # the features' cells carry what they claim
    for b, s in enumerate(scenes):
        for f, (v, c), fv, fl in cs.claimed(s, case.rflag):
            assert fv is None or got_fv[b, v, c] == fv, (case.id, f.name, v, c, "flagV")
            assert fl is None or got_flag[b, v, c] == fl, (case.id, f.name, v, c, "flag")
    # without a flagV output (the context's scratch plane instead): the same flags
    raw_f2, d_flag2 = guarded(torch, shape, torch.uint8)
    eng.cfar_dev(d_x, d_flag2, None, cfar=cf)
    torch.cuda.synchronize()
    assert (check_guards(raw_f2, shape).reshape(shape) == got_flag).all()


@pytest.mark.gpu
def test_window_past_the_built_range_is_refused(torch_cuda, cfar_engine):
    """ref + guard = 31 cells is one more than the range kernels' halo holds: RSP_ERR_UNSUPPORTED
    from the call and from the plan, and nothing written."""
    torch = torch_cuda
    from rsp import RspError
    cf = cfar_obj((16, 14, 17, 14), 3.0, 0, 0, [], (0, 0))
    with pytest.raises(RspError) as ei:
        cfar_engine.cfar_plan(cf, 2, V=64, R=272, fused=False)
    assert ei.value.code == 3
    d_x = torch.ones((2, 64, 272), dtype=torch.float32, device="cuda")
    raw, d_flag = guarded(torch, (2, 64, 272), torch.uint8)
    with pytest.raises(RspError) as ei:
        cfar_engine.cfar_dev(d_x, d_flag, None, cfar=cf)
    assert ei.value.code == 3
    torch.cuda.synchronize()
    assert (raw.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------------------------ (b) fused
KAISER, HAMMING, RECT = 0, 1, 2
# MTD tile per pulse count: rows per thread E (24 for 3 * 2^k, else 16), G = P / E threads per range
# bin, T threads per workgroup (256; from P = 512 on 16 * G up to 1024), W = T / G range bins.
# Bluestein (P = 83): the tile of its NF = 256-point transform, regions of W * P entries.
TILE = {32: (128, 256, 16), 48: (128, 256, 24), 64: (64, 256, 16), 128: (32, 256, 16), 192: (32, 256, 24),
        512: (16, 512, 16), 83: (16, 256, 16)}
BLUESTEIN = {83: 256}


@dataclasses.dataclass(frozen=True)
class F:
    """rsp_mtd_cfar_dev on 5 CPIs of [P][R].  M0 against the E rows of a thread's first run: inside
    it, lo on its boundary (M0 = E - 1), hi on one (M0 = E), past it (M0 = E + 3), where the band
    still holds 2 * (ref + guard) rows.  dense_T: the lower threshold, 1.5 unless the band or the
    tile is too small for a tile's hits to outnumber the workgroup's threads at 1.5."""
    id: str
    P: int
    R: int
    M0: int
    nseg: int
    mtd_zdiv: int
    zdiv: int
    methods: tuple
    win: tuple = W57
    window: int = KAISER
    dense_T: float = 1.5


FUSED = [
    # ---- the 5 + 7 window (compiled into the MTD kernel) on every pulse count; R = max(2W + 5, 101)
    # is odd with a ragged last tile, the other R a multiple of 16
    F("p32-odd", 32, 261, 3, 0, 150, 20, (0, 0)),
    F("p32-r16", 32, 272, 0, 4, 0, 0, (1, 1)),
    F("p48-odd-m0max", 48, 261, 11, 4, 0, 20, (0, 1), dense_T=1.3),
    F("p48-r16", 48, 272, 2, 0, 150, 0, (1, 0)),
    F("p64-odd-inside", 64, 133, 3, 3, 150, 20, (0, 0)),
    F("p64-odd-lo-on-run", 64, 133, 15, 0, 0, 0, (1, 1), dense_T=1.25),
    F("p64-r16-hi-on-run", 64, 144, 16, 3, 0, 20, (0, 1), dense_T=1.25),
    F("p64-odd-past-run", 64, 133, 19, 1, 150, 0, (1, 0), dense_T=1.15),
    F("p128-odd-inside", 128, 101, 5, 0, 150, 20, (0, 0)),
    F("p128-odd-lo-on-run", 128, 101, 15, 3, 0, 0, (0, 1)),
    F("p128-r16-hi-on-run", 128, 112, 16, 0, 150, 20, (1, 0)),
    F("p128-odd-past-run", 128, 101, 19, 1, 0, 20, (1, 1)),
    F("p192-odd-inside", 192, 101, 5, 0, 150, 20, (0, 0)),
    F("p192-odd-lo-on-run", 192, 101, 23, 3, 0, 0, (1, 1)),
    F("p192-r16-hi-on-run", 192, 112, 24, 0, 0, 20, (0, 1)),
    F("p192-odd-past-run", 192, 101, 27, 1, 150, 0, (1, 0)),
    F("p512-odd-inside", 512, 101, 5, 0, 150, 20, (0, 0)),
    F("p512-r16-lo-on-run", 512, 112, 15, 3, 0, 0, (1, 1)),
    F("p512-odd-past-run", 512, 101, 19, 1, 0, 20, (0, 1)),
    F("bluestein83-odd", 83, 101, 3, 0, 150, 20, (0, 0), dense_T=1.25),
    F("bluestein83-r16", 83, 112, 0, 3, 0, 0, (1, 1), dense_T=1.25),
    # ---- other windows: the runtime-window MTD instance (5 reference cells with another guard too)
    F("p64-w5-4", 64, 133, 3, 0, 150, 20, (0, 0), (5, 4, 5, 4)),
    F("p64-w3-2", 64, 144, 15, 3, 0, 0, (1, 1), (3, 2, 3, 2)),
    F("p64-w8-4", 64, 133, 16, 1, 0, 20, (0, 1), (8, 4, 8, 4), dense_T=1.25),
    F("p128-w5-4", 128, 101, 15, 3, 0, 0, (1, 0), (5, 4, 5, 4)),
    F("p128-w3-2", 128, 112, 5, 0, 150, 20, (0, 0), (3, 2, 3, 2)),
    F("p128-w8-4", 128, 101, 19, 0, 0, 20, (1, 1), (8, 4, 8, 4)),
    F("p192-w5-4", 192, 101, 23, 0, 0, 0, (0, 1), (5, 4, 5, 4)),
    F("p192-w3-2", 192, 101, 27, 3, 0, 20, (1, 0), (3, 2, 3, 2)),
    F("p192-w8-4", 192, 112, 5, 0, 150, 20, (0, 0), (8, 4, 8, 4)),
    # ---- the other slow-time windows (the RDM guard below is what checks them)
    F("p128-rect", 128, 101, 5, 0, 150, 20, (0, 0), window=RECT),
    F("p128-hamming", 128, 101, 5, 3, 0, 20, (1, 1), window=HAMMING),
]
BATCH = 5


def fused_T(case, dense):
    return case.dense_T if dense else 3.0


def fused_plan(case, mode):
    """The plan of one call mode, by the rules: chunk = 2 cuts 5 CPIs into 2 + 2 + 1 on two pipelines
    (the last, short chunk on the first); chunk = 5 is one chunk.  With an RDM output the range stages
    run grouped (16 chunks per group: one partial group per pipeline); without one (chunk = 2) the
    first chunk's stage rides in its pipeline's next MTD launch -- RangeJob57 where the Doppler window
    is compiled in and the range window is 5 + 7, prev_chunk_hits otherwise (Bluestein included).
    Hit kernel of the separate launches: 5 + 7 regions of 64 .. 4096 entries the batched kernel at 16
    lanes per region (V <= 128), larger ones at 256; any other window the per-hit runtime kernel."""
    W, T, _ = TILE[case.P]
    w57 = case.win[2:] == (5, 7)
    compiled = case.win[:2] == (5, 7) and case.P not in BLUESTEIN
    region = W * case.P
    if mode == "rflag0":
        stage, kern, lanes = NONE, H_NONE, 0
    else:
        kern = H_BATCHED57 if w57 else H_RUNTIME
        lanes = 0 if not w57 else (16 if region <= 4096 else 256)
        stage = JOB57 if compiled and w57 else PREV_HITS
        if mode != "chunk2-nordm":
            stage = GROUPED
    one = mode == "chunk5"
    return dict(fused=1, window_compiled=int(compiled), bluestein=BLUESTEIN.get(case.P, 0), tile_w=W, threads=T,
                region=region, nchunks=1 if one else 3, nlanes=1 if one else 2,
                lane_chunk=[5] if one else [2, 2], lane_last=[5] if one else [1, 2], range_stage=stage,
                hit_kernel=kern, hit_lanes=lanes, flag_memset=0)


def slow_time_window(case):
    if case.window == RECT:
        return np.ones(case.P)
    return ref.hamming(case.P) if case.window == HAMMING else ref.kaiser(case.P, 8.0)


def fused_scenes(case):
    return [scene(case.P, case.R, case.nseg, case.M0, case.zdiv, case.win, case.mtd_zdiv, cs.SEED + b)
            for b in range(BATCH)]


def fused_spec(case):
    from test_gpu_pc_geometry import MF, seg_spec
    spec = seg_spec(case.R, case.R, [(MF, 0, case.R, 0, case.R, 512, 67)])(case.P)
    return dataclasses.replace(spec, zero_v_div=case.mtd_zdiv, window=case.window)


@pytest.mark.gpu
@pytest.mark.parametrize("dense", (False, True), ids=("T3", "dense"))
@pytest.mark.parametrize("case", FUSED, ids=lambda c: c.id)
def test_fused(torch_cuda, case, dense):
    torch = torch_cuda
    from rsp.engine import Engine
    scenes = fused_scenes(case)
    segs = scenes[0].segments
    T = fused_T(case, dense)
    cf = cfar_obj(case.win, T, case.M0, case.zdiv, segs, case.methods)
    cf0 = dataclasses.replace(cf, rFlag=0)
    rng = np.random.default_rng(cs.SEED)
    w = slow_time_window(case)
    pc = np.stack([cs.to_pc(s.field, w, rng) for s in scenes])
    d_pc = torch.from_numpy(pc).cuda()
    shape = (BATCH, case.P, case.R)
    W, threads, _ = TILE[case.P]
    eng = Engine(fused_spec(case), device=0, chunk=2)

    def run(cfar, rdm=True, flagv=True):
        raw_r, d_rdm = guarded(torch, shape, torch.float32) if rdm else (None, None)
        raw_f, d_flag = guarded(torch, shape, torch.uint8)
        raw_v, d_fv = guarded(torch, shape, torch.uint8) if flagv else (None, None)
        eng.mtd_dev(d_pc, rdm=d_rdm, flag=d_flag, flagV=d_fv, cfar=cfar)
        torch.cuda.synchronize()
        out_r = check_guards(raw_r, shape, 4).view(np.float32).reshape(shape) if rdm else None
        out_v = check_guards(raw_v, shape).reshape(shape) if flagv else None
        return out_r, check_guards(raw_f, shape).reshape(shape), out_v

    try:
        # chunk = 2 with an RDM output: grouped launches, a partial group on either pipeline
        assert eng.cfar_plan(cf, BATCH) == fused_plan(case, "chunk2")
        rdm, flag, fv = run(cf)
        # the scene landed: the RDM is the designed field (exact zeros on the MTD's zeroed rows)
        want = np.stack([s.field for s in scenes])
        zr = np.zeros(case.P, bool)
        if case.mtd_zdiv:
            a, b = ref.zero_v_rows(case.P, case.mtd_zdiv)
            zr[a:b] = True
        assert not rdm[:, zr].any()
        err = np.linalg.norm(rdm[:, ~zr] - want[:, ~zr]) / np.linalg.norm(want[:, ~zr])
        print("%s: RDM against the designed field %.2e" % (case.id, err))
        assert err < RDM_TOL
        oflag, oflagV, amb = check_flags(flag, fv, rdm.astype(np.float64), cf, scenes, case.id + " chunk2")
        if dense:   # the in-launch job below must run past its first pass: a tile of the first (full)
            # chunk with more Doppler hits than the workgroup has threads
            ntile = -(-case.R // W)
            per_tile = [int(oflagV[b, :, t * W:(t + 1) * W].sum()) for b in range(2) for t in range(ntile)]
            print("%s: Doppler hits per tile of chunk 0: max %d, threads %d" % (case.id, max(per_tile), threads))
            assert max(per_tile) > threads
        # chunk = 2 without an RDM output: the first chunk's range stage inside the short last chunk's
        # MTD launch (more regions than that launch has workgroups); bit-equal flags
        assert eng.cfar_plan(cf, BATCH, rdm=False) == fused_plan(case, "chunk2-nordm")
        _, flag_n, fv_n = run(cf, rdm=False)
        assert (flag_n == flag).all() and (fv_n == fv).all()
        # ... and without a flagV output either
        _, flag_q, _ = run(cf, rdm=False, flagv=False)
        assert (flag_q == flag).all()
        _, flag_q, _ = run(cf, flagv=False)
        assert (flag_q == flag).all()
        # rFlag = 0: the MTD launch alone, flag = flagV
        assert eng.cfar_plan(cf0, BATCH) == fused_plan(case, "rflag0")
        rdm0, flag0, fv0 = run(cf0)
        assert (rdm0 == rdm).all() and (fv0 == fv).all() and (flag0 == fv).all()
        # one chunk of 5
        eng.set_chunk(5)
        assert eng.cfar_plan(cf, BATCH) == fused_plan(case, "chunk5")
        rdm5, flag5, fv5 = run(cf)
        assert (rdm5 == rdm).all() and (flag5 == flag).all() and (fv5 == fv).all()
    finally:
        eng.close()
