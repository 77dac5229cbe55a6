#!/usr/bin/env python3
"""Plot condensation throughput on the measurement bench's shape: the 2048 x 512 DMX long part
as the column window (62, 574) of ld = 574 planes, batch 256, planes resident in HBM.  Two
scenes: ~0.1 % of cells flagged (about 1044 hits per CPI, bench.py --config measure) and 5.7 %
(what the c5 chain flags).  Timed in one process with HIP events, each variant after a warm-up
of at least 3 steps and 0.3 s, in alternating rounds so that the spread between rounds is seen
next to the differences:

  1. rsp_condense_dev                                   (dense bytes: flag read + peak written)
  2. rsp_motion_measure_dev on the CFAR flags           (today: every hit listed and measured)
  3. (1) + rsp_motion_measure_dev on the peak plane     (one estimate per plot)
  4. the condensation as a torch composition: labels by iterated 3 x 3 max-pool propagation to
     a fixed point, peaks by scatter_reduce (a smaller batch; time scaled per CPI)

Rates: dense bytes (2 B per cell of the window) over the event time, also as a fraction of the
6.24 TB/s copy ceiling (profiles/hbm_ceiling.json).
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "radar-signal-process_amd")]

CEILING = 6.24e12


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


def torch_condense(amp, flag):
    """[B][V][R] -> (peak uint8, n_plots per CPI): 8-connectivity, no wrap, first maximum in
    find() order.  Labels are cell numbers + 1 in float32 (exact below 2^24)."""
    import torch
    import torch.nn.functional as F
    B, V, R = flag.shape
    on = flag != 0
    idx = torch.arange(1, V * R + 1, device=flag.device, dtype=torch.float32).reshape(1, V, R)
    lab = torch.where(on, idx, torch.zeros((), device=flag.device))
    while True:
        new = torch.where(on, F.max_pool2d(lab[:, None], 3, 1, 1)[:, 0], lab)
        if torch.equal(new, lab):
            break
        lab = new
    li = lab.long().reshape(B, -1)
    a = torch.where(on, amp, torch.full((), -1.0, device=flag.device)).reshape(B, -1)
    top = torch.full((B, V * R + 1), -1.0, device=flag.device).scatter_reduce(1, li, a, "amax")
    # candidates: the cells that hold their label's maximum; the first in find() order wins
    key = (torch.arange(R, device=flag.device)[None, :] * V + torch.arange(V, device=flag.device)[:, None]).reshape(1, -1)
    cand = on.reshape(B, -1) & (a == top.gather(1, li))
    big = V * R
    k = torch.where(cand, key.expand(B, -1), torch.full((), big, device=flag.device))
    first = torch.full((B, V * R + 1), big, device=flag.device).scatter_reduce(1, li, k, "amin")
    peak = (cand & (k == first.gather(1, li))).reshape(B, V, R).to(torch.uint8)
    return peak, peak.reshape(B, -1).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--torch-batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from rsp import condense, measure
    if not torch.cuda.is_available():
        sys.exit("condense_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    B, V, Rp, lo, hi = a.batch, 2048, 574, 62, 574
    R = hi - lo
    M0 = 6
    g = torch.Generator(device=dev)
    g.manual_seed(4000)
    s = torch.rand((B, V, Rp), generator=g, device=dev) * 2 + 0.1
    d = torch.randn((B, V, Rp), generator=g, device=dev) * 0.5
    cond, meas = condense.Condense(0), measure.Measure(0)
    kv = measure.angle_KvalueGen(1)
    p = meas.params(2, 5.996, 8, 0.2, 4, kv[4, 3], 3, 5.0, 0.0, 0.0, M0)
    p.ld, p.cpi_stride = Rp, V * Rp
    rs = torch.as_tensor(np.arange(R) * 5.996, device=dev)
    vs = torch.as_tensor(-(np.arange(V) - V / 2) * 0.2, device=dev)
    from rsp import _capi as capi
    cp = capi.rsp_condense_params()
    cp.gap_v, cp.gap_r, cp.wrap_v, cp.ld, cp.cpi_stride = 1, 1, 0, Rp, V * Rp
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    peak = torch.zeros((B, V, Rp), dtype=torch.uint8, device=dev)
    count = torch.empty((B, 2), dtype=torch.int32, device=dev)
    mcount = torch.empty((B, 2), dtype=torch.int32, device=dev)
    print("shape: %d CPIs, %d x %d window at column %d of ld = %d planes" % (B, V, R, lo, Rp), flush=True)
    for density in (1e-3, 0.057):
        f = (torch.rand((B, V, Rp), generator=g, device=dev) < density).to(torch.uint8)
        f[:, :M0 + 1, :] = 0
        f[:, V - M0:, :] = 0
        hits = float(f[:, :, lo:hi].sum()) / B
        max_hits = 4096 if hits < 3000 else 1 << 17
        est = torch.empty((B, max_hits, 3), dtype=torch.float64, device=dev)
        cells = torch.empty((B, max_hits, 2), dtype=torch.int32, device=dev)
        plots = torch.empty((B, max_hits, 8), dtype=torch.int32, device=dev)

        def run_condense():
            rc = cond.lib.rsp_condense_dev(cond.ctx, s.data_ptr() + 4 * lo, f.data_ptr() + lo, V, R, B, C.byref(cp),
                                           peak.data_ptr() + lo, max_hits, plots.data_ptr(), count.data_ptr(), st)
            assert rc == 0

        def measure_on(flags):
            rc = meas.lib.rsp_motion_measure_dev(meas.ctx, s.data_ptr() + 4 * lo, d.data_ptr() + 4 * lo,
                                                 flags.data_ptr() + lo, V, R, B, C.byref(p), rs.data_ptr(), vs.data_ptr(),
                                                 max_hits, est.data_ptr(), cells.data_ptr(), mcount.data_ptr(), st)
            assert rc == 0

        def run_measure_all():
            measure_on(f)

        def run_condense_measure():
            run_condense()
            measure_on(peak)

        tb = min(a.torch_batch, B)
        sw, fw = s[:tb, :, lo:hi].contiguous(), f[:tb, :, lo:hi].contiguous()

        def run_torch():
            torch_condense(sw, fw)

        cases = [("1 rsp_condense_dev", run_condense, B), ("2 measure every hit (today)", run_measure_all, B),
                 ("3 condense + measure the peaks", run_condense_measure, B),
                 ("4 torch composition of 1 (batch %d)" % tb, run_torch, tb)]
        for _, fn, _ in cases:
            warm(fn)
        # like for like: the torch composition finds the same peaks
        run_condense()
        tp, tn = torch_condense(sw, fw)
        torch.cuda.synchronize()
        same = bool(torch.equal(tp, peak[:tb, :, lo:hi])) and bool(torch.equal(tn.int(), count[:tb, 0]))
        n_plots = float(count[:, 0].double().mean())
        assert int(count[:, 0].max()) <= max_hits
        print("\ndensity %.3g: %.0f hits, %.0f plots per CPI; torch peaks equal on %d CPIs: %s"
              % (density, hits, n_plots, tb, same), flush=True)
        times = {name: [] for name, _, _ in cases}
        for _ in range(a.rounds):
            for name, fn, _ in cases:
                times[name].append(timed(fn, a.iters if "torch" not in name else max(1, a.iters // 5)))
        print("%-38s %10s %10s %10s %12s %9s %8s" % ("", "median ms", "min ms", "max ms", "CPI/s", "dense TB/s", "of 6.24"))
        med = {}
        for name, _, nb in cases:
            t = sorted(times[name])
            med[name] = t[len(t) // 2] / nb
            rate = 2.0 * V * R / med[name]
            dense = "%9.3f %7.1f%%" % (rate / 1e12, 100.0 * rate / CEILING) if name[0] in "14" else ""
            print("%-38s %10.3f %10.3f %10.3f %12.0f %s" % (name, t[len(t) // 2] * 1e3, t[0] * 1e3, t[-1] * 1e3,
                                                         1.0 / med[name], dense), flush=True)
        n1, n2, n3, n4 = (c[0] for c in cases)
        print("condense + measure peaks / measure every hit: %.2fx the time; torch / rsp_condense_dev per CPI: %.1fx"
              % (med[n3] / med[n2], med[n4] / med[n1]), flush=True)
        del f, est, cells, plots


if __name__ == "__main__":
    main()
