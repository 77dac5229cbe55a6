#!/usr/bin/env python3
"""Doppler line width throughput (rsp_spec_width_dev) on the measurement bench's
shape: the 2048 x 512 DMX long part as the column window (62, 574) of ld = 574 planes, batch 256,
planes resident in HBM (1.2 GB of amplitudes).  Amplitudes: Rayleigh noise plus one line of a few
bins per column.  Two hit densities: 0.1 % of cells flagged (about 1044 hits per CPI, bench.py
--config measure; independent random cells, so most columns carry one) and every column
(d_flag = NULL); interp 1 and 8; level -6 dB, shift = 1.

Timed in one process with HIP events, each variant after a warm-up of at least 3 calls and 0.3 s,
in alternating rounds so that the spread between rounds is seen next to the differences:

  1-4. rsp_spec_width_dev at (density, interp)
  5.   rsp_motion_measure_dev on the same planes and flags, for scale

Bytes read: the flag window (V * R bytes per CPI, when flags are given) plus 4 * V bytes per
computed column, over the whole call's event time, also as a share of the 7.23 TB/s read ceiling
(profiles/hbm_ceiling.json).  The stage is not a streaming kernel: the share says how far from a
memory bound it runs, not how well it streams.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "radar-signal-process_amd")]

CEILING = 7.2335e12


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def warm(fn, seconds=0.3):
    import torch
    t0 = time.perf_counter()
    n = 0
    while n < 3 or time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()
        n += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from rsp import _capi as capi
    from rsp import measure, width
    if not torch.cuda.is_available():
        sys.exit("width_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    B, V, Rp, lo, hi = a.batch, 2048, 574, 62, 574
    R = hi - lo
    M0 = 6
    g = torch.Generator(device=dev)
    g.manual_seed(4200)
    s = torch.view_as_complex(torch.randn((B, V, Rp, 2), generator=g, device=dev)).abs()
    v0 = torch.rand((B, 1, Rp), generator=g, device=dev) * V
    for v in range(0, V, 256):     # the line, in slabs of rows (no [B][V][Rp] temporaries beyond one slab)
        dv = (torch.arange(v, v + 256, device=dev, dtype=torch.float32)[None, :, None] - v0 + V / 2) % V - V / 2
        s[:, v:v + 256] += 40.0 * torch.exp(-0.5 * (dv / 1.5) ** 2)
    del dv
    s[:, :M0 + 1, :] = 0
    s[:, V - M0:, :] = 0
    d = torch.randn((B, V, Rp), generator=g, device=dev) * 0.5
    f = (torch.rand((B, V, Rp), generator=g, device=dev) < 1e-3).to(torch.uint8)
    f[:, :M0 + 1, :] = 0
    f[:, V - M0:, :] = 0
    hits = float(f[:, :, lo:hi].sum()) / B
    wd, meas = width.Width(0), measure.Measure(0)
    kv = measure.angle_KvalueGen(1)
    p = meas.params(2, 5.996, 8, 0.2, 4, kv[4, 3], 3, 5.0, 0.0, 0.0, M0)
    p.ld, p.cpi_stride = Rp, V * Rp
    rs = torch.as_tensor(np.arange(R) * 5.996, device=dev)
    vs = torch.as_tensor(-(np.arange(V) - V / 2) * 0.2, device=dev)
    max_hits = 4096
    est = torch.empty((B, max_hits, 3), dtype=torch.float64, device=dev)
    cells = torch.empty((B, max_hits, 2), dtype=torch.int32, device=dev)
    mcount = torch.empty((B, 2), dtype=torch.int32, device=dev)
    span = torch.empty((B, R, 2), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def width_case(flags, interp):
        wp = capi.rsp_width_params()
        wp.amp_constr, wp.interp, wp.shift, wp.ld, wp.cpi_stride = -6.0, interp, 1, Rp, V * Rp

        def run():
            rc = wd.lib.rsp_spec_width_dev(wd.ctx, s.data_ptr() + 4 * lo, flags.data_ptr() + lo if flags is not None else None,
                                           V, R, B, C.byref(wp), span.data_ptr(), count.data_ptr(), st)
            assert rc == 0
        return run

    def run_measure():
        rc = meas.lib.rsp_motion_measure_dev(meas.ctx, s.data_ptr() + 4 * lo, d.data_ptr() + 4 * lo, f.data_ptr() + lo, V, R,
                                             B, C.byref(p), rs.data_ptr(), vs.data_ptr(), max_hits, est.data_ptr(),
                                             cells.data_ptr(), mcount.data_ptr(), st)
        assert rc == 0

    cases = []
    for interp in (1, 8):
        for name, flags in (("0.1 % flagged", f), ("every column", None)):
            fn = width_case(flags, interp)
            fn()
            torch.cuda.synchronize()
            cols = float(count.double().mean())
            wdots = width.width_dots(span, interp)
            mean_w = float(wdots[span[..., 0] >= 0].mean())
            nbytes = (V * R if flags is not None else 0) + 4.0 * V * cols
            cases.append(("rsp_spec_width_dev " + name + " interp " + str(interp), fn, cols, nbytes, mean_w))
    cases.append(("rsp_motion_measure_dev (0.1 % flagged)", run_measure, None, None, None))
    print("shape: %d CPIs, %d x %d window at column %d of ld = %d planes; %.0f hits per CPI at 0.1 %%; level -6 dB, shift 1"
          % (B, V, R, lo, Rp, hits), flush=True)
    for c in cases:
        warm(c[1])
    times = {c[0]: [] for c in cases}
    for _ in range(a.rounds):
        for c in cases:
            times[c[0]].append(timed(c[1], a.iters))
    print("%-48s %9s %8s %8s %9s %10s %11s %8s %8s %9s" % ("", "median ms", "min ms", "max ms", "CPI/s", "cols/CPI",
                                                          "columns/s", "TB/s", "of 7.23", "widthDots"))
    med = {}
    for name, _, cols, nbytes, mean_w in cases:
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        line = "%-48s %9.3f %8.3f %8.3f %9.0f" % (name, med[name] * 1e3, t[0] * 1e3, t[-1] * 1e3, B / med[name])
        if cols is not None:
            rate = nbytes * B / med[name]
            line += " %10.1f %11.3g %8.3f %7.1f%% %9.2f" % (cols, cols * B / med[name], rate / 1e12, 100.0 * rate / CEILING,
                                                          mean_w)
        print(line, flush=True)
    ref = med[cases[-1][0]]
    for name, _, cols, _, _ in cases[:-1]:
        print("%s / rsp_motion_measure_dev: %.2fx the time" % (name, med[name] / ref), flush=True)
    wd.close()
    meas.close()


if __name__ == "__main__":
    main()
