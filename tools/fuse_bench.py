#!/usr/bin/env python3
"""Stacked-beam fusion throughput (rsp_beam_fuse_dev) beside the same result as a torch
composition (masked amax / argmax / count) on the same planes, resident in HBM:

  v2 capture   13 beams x 332 rows x the v2 preset's R_out, batch 8   (Engine.window_dev's layout:
  c4           13 beams x 256 rows x 8192,                  batch 4    beam outermost, read through the view)

The batches are chosen so that the planes (beams x 5 B per cell) exceed the 256 MiB Infinity Cache.  Flags
at the sparse density of a CFAR on noise (1e-3 per beam) and at 5.7 % per beam.  All four outputs are
written.  The torch composition is checked to give the same bytes once, before the timing.

Timed in one process with HIP events, every variant after a warm-up of at least 3 calls and 0.3 s, in
alternating rounds (5 rounds of 5 calls by default, the median reported) so that the spread between rounds is
seen next to the differences.  Bytes moved: beams x 5 read + 7 written per cell, as a rate and as a share of
the 7.23 TB/s read ceiling (profiles/hbm_ceiling.json).

RSP_FUSE_GROUP=4 in the environment makes the kernel issue the loads of four beams before the first compare
instead of one beam's at a time (read once per process): run the tool alternately with and without it,
--no-torch, for that A/B.

The last line times rsp_beam_elev_dev once, at 1000 listed hits per CPI under law 2.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "radar-signal-process_amd")]

READ_CEILING = 7.2335e12
X13 = np.cumsum([0.0, 2.1, 1.8, 2.3, 1.9, 2.0, 2.4, 1.7, 2.2, 1.95, 2.05, 1.85, 2.15]) - 3.0


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


def torch_fuse(amp, flag, min_beams, out):
    """The same four planes from torch ops: masked amax / argmax / count over the beam axis."""
    import torch
    f = flag != 0
    cnt = f.sum(1)
    hit = cnt >= min_beams
    peak = torch.where(f, amp, torch.full((), -float("inf"), device=amp.device)).argmax(1)   # the first of equal maxima
    out[0].copy_(hit)
    out[1].copy_(torch.where(hit, peak, torch.full_like(peak, 255)))
    torch.amax(amp, 1, out=out[2])
    out[3].copy_(cnt)


def bench(a):
    import torch
    from rsp import presets
    from rsp.fuse import BeamFuser
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(4500)
    K = 13
    shapes = [("v2 capture", max(1, int(8 * a.scale)), 332, presets.v2().R_out), ("c4", max(1, int(4 * a.scale)), 256, 8192)]
    print("%d iterations x %d rounds per variant; loads issued per thread before the first compare: %s beam(s)"
          % (a.iters, a.rounds, "4" if os.environ.get("RSP_FUSE_GROUP", "")[:1] == "4" else "1"), flush=True)
    fuser = BeamFuser(X13, min_beams=2, device=0)
    for name, B, V, R in shapes:
        # Engine.window_dev's layout [beams][batch][V][R], fused through the view
        rdm = torch.randn((K, B, V, R), generator=g, device=dev).abs_()
        amp = rdm.transpose(0, 1)
        print("\n%s: %d CPIs of %d beams x %d x %d, %.0f MiB of planes per batch" % (name, B, K, V, R, K * B * V * R * 5 / 2 ** 20),
              flush=True)
        dts = (torch.uint8, torch.uint8, torch.float32, torch.uint8)
        out = tuple(torch.empty((B, V, R), dtype=dt, device=dev) for dt in dts)
        out_t = tuple(torch.empty((B, V, R), dtype=dt, device=dev) for dt in dts)
        cases = []
        for density in (1e-3, 0.057):
            flg = (torch.rand((K, B, V, R), generator=g, device=dev) < density).to(torch.uint8).transpose(0, 1)
            fuser.fuse_dev(amp, flg, out=out)
            hits = float(out[0].sum().item()) / B
            same = "not run"
            if not a.no_torch:
                torch_fuse(amp, flg, 2, out_t)
                torch.cuda.synchronize()
                same = all(bool((x == y).all().item()) for x, y in zip(out, out_t))
            print("density %.3g per beam: %.0f fused hits per CPI (min_beams 2); torch composition equal: %s" % (density, hits, same),
                  flush=True)
            cases.append(("rsp_beam_fuse_dev  density %.3g" % density, lambda flg=flg: fuser.fuse_dev(amp, flg, out=out)))
            if not a.no_torch:
                cases.append(("torch composition density %.3g" % density, lambda flg=flg: torch_fuse(amp, flg, 2, out_t)))
        for c in cases:
            warm(c[1])
        times = {c[0]: [] for c in cases}
        for _ in range(a.rounds):
            for c in cases:
                times[c[0]].append(timed(c[1], a.iters))
        print("%-40s %9s %8s %8s | %9s | %7s %7s | %s" % ("", "median ms", "min ms", "max ms", "cells/s", "TB/s", "of 7.23", "x kernel"))
        med = {}
        for cname, _ in cases:
            t = sorted(times[cname])
            med[cname] = t[len(t) // 2]
        for cname, _ in cases:
            t = sorted(times[cname])
            m = med[cname]
            rate = (K * 5 + 7.0) * B * V * R / m
            base = med[cname.replace("torch composition", "rsp_beam_fuse_dev ")]
            print("%-40s %9.3f %8.3f %8.3f | %9.3e | %7.3f %6.1f%% | %6.2f"
                  % (cname, m * 1e3, t[0] * 1e3, t[-1] * 1e3, B * V * R / m, rate / 1e12, 100 * rate / READ_CEILING, m / base),
                  flush=True)
        if name == "c4" and not a.no_elev:
            elev_line(fuser, amp, B, V, R, g)
        del rdm, amp, out, out_t, cases
    fuser.close()


def elev_line(fuser, amp, B, V, R, g):
    import torch
    dev = amp.device
    H = 1000
    flg = (torch.rand((13, B, V, R), generator=g, device=dev) < 0.057).to(torch.uint8).transpose(0, 1)
    fbeam = torch.randint(1, 12, (B, V, R), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)   # every cell an interior peak
    cells = torch.stack([torch.randint(0, V, (B, H), generator=g, device=dev, dtype=torch.int32),
                         torch.randint(0, R, (B, H), generator=g, device=dev, dtype=torch.int32)], dim=2).contiguous()
    count = torch.tensor([[H, 0]] * B, dtype=torch.int32, device=dev)
    est = torch.zeros((B, H, 3), dtype=torch.float64, device=dev)
    hb = torch.empty((B, H, 4), dtype=torch.int32, device=dev)
    fn = lambda: fuser.elevation_dev(amp, flg, fbeam, cells, count, est=est, hb=hb)   # noqa: E731
    warm(fn)
    t = sorted(timed(fn, 20) for _ in range(5))
    print("\nrsp_beam_elev_dev, law 2, %d CPIs x %d hits into est[..][2] with d_hb: median %.1f us per call (min %.1f, max %.1f)"
          % (B, H, t[2] * 1e6, t[0] * 1e6, t[-1] * 1e6), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the batches (a quick look: 0.25)")
    ap.add_argument("--no-torch", action="store_true", help="the kernel alone (the A/B of RSP_FUSE_GROUP)")
    ap.add_argument("--no-elev", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fuse_bench: needs a GPU")
    bench(a)


if __name__ == "__main__":
    main()
