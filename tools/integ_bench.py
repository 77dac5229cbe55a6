#!/usr/bin/env python3
"""Post-detection integration throughput (rsp_integrate_dev) beside the same thing as a
torch composition (pad, gather, add) on the same planes, resident in HBM:

  c3         128 x 4096 planes, batch 256 (ld = R)
  dmx long   2048 x 512, the column window (62, 574) of ld = 574 planes, batch 96

The sum form at n = 2, 4, 8, without shifts (d_shift NULL) and with a walk table (DMX: walk_shifts of the
preset's vScale at the 80 ms frame time; c3: a ramp of -3 .. +3 columns per CPI over the rows).  The ring
is in its steady state (every CPI sums n planes).  The torch composition sums the same planes for one
slot from a cold ring (CPI b adds CPIs b-1 .. b-n+1 of the batch), which is less work.

Timed in one process with HIP events, every variant after a warm-up of at least 3 calls and 0.3 s, in
alternating rounds so that the spread between rounds is seen next to the differences.  Bytes moved are
counted twice: as 1 read + 1 write per cell (8 B: what has to cross the HBM interface if every re-read
hits a cache) and as n reads + 1 write (4 (n + 1) B: what the kernel asks for), each as a rate and as a
share of the 7.23 TB/s read and 6.24 TB/s copy ceilings (profiles/hbm_ceiling.json).

--scr adds one Pd-versus-SCR line (rsp.score.scr_sweep): the synthetic DMX preset (128 x 4096), one
injected target per CPI that moves two range cells from CPI to CPI, the chain's CFAR on the single CPI
against the same CFAR behind an n = 4 sum without and with walk compensation.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "radar-signal-process_amd")]

READ_CEILING = 7.2335e12
COPY_CEILING = 6.24e12


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


def torch_sum(x, lo, hi, n, shift, out):
    """The same sums from torch ops, one slot from a cold ring: pad (the out-of-window zero), gather, add."""
    import torch
    w = x[:, :, lo:hi]
    B, V, R = w.shape
    o = out[:, :, lo:hi]
    o.copy_(w)
    for i in range(1, min(n, B)):
        if shift is None:
            o[i:] += w[:B - i]
            continue
        src = torch.arange(R, device=x.device)[None, :] - shift[i - 1].to(torch.int64)[:, None]     # [V][R]
        idx = torch.where((src >= 0) & (src < R), src, torch.full_like(src, R))                      # R: the pad column
        padded = torch.nn.functional.pad(w[:B - i], (0, 1))
        o[i:] += torch.gather(padded, 2, idx[None].expand(B - i, V, R))


def bench(a):
    import torch
    from rsp import dmx, presets
    from rsp.integrate import Integrator, walk_shifts
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(4400)
    B3 = max(8, int(256 * a.scale))
    Bd = max(8, int(96 * a.scale))
    spec = presets.dmx_native()
    vS, dR = dmx.dmx_scales(spec, 0)[2:4]
    shapes = [("c3 128x4096", (B3, 128, 4096), 0, 4096,
               lambda n: np.rint(np.arange(1, n)[:, None] * np.linspace(-3.0, 3.0, 128)[None, :]).astype(np.int32)),
              ("dmx long 2048x512", (Bd, 2048, 574), 62, 574,
               lambda n: walk_shifts(vS, spec.P * presets.DMX_PRT, dR, n))]
    print("%d iterations x %d rounds per variant" % (a.iters, a.rounds), flush=True)
    for name, shp, lo, hi, table in shapes:
        B, V, Rp = shp
        R = hi - lo
        x = torch.randn(shp, generator=g, device=dev).abs_()
        out = torch.zeros(shp, dtype=torch.float32, device=dev)
        print("\n%s: %d CPIs, %d x %d window at column %d of ld = %d, %.0f MiB per batch of planes"
              % (name, B, V, R, lo, Rp, B * V * R * 4 / 2 ** 20), flush=True)
        cases = []
        keep = []
        for n in (2, 4, 8):
            for walk in (False, True):
                sh = table(n) if walk else None
                d_sh = None if sh is None else torch.from_numpy(sh).to(dev)
                integ = Integrator(0, n=n)
                keep.append(integ)
                cols = None if (lo, hi) == (0, Rp) else (lo, hi)
                label = "n=%d %s" % (n, "walk |s|<=%d" % int(np.abs(sh).max()) if walk else "no shift")
                cases.append(("rsp_integrate_dev " + label, n,
                              lambda integ=integ, d_sh=d_sh, cols=cols: integ.sum_dev(x, shift=d_sh, cols=cols, out=out)))
                if not a.no_torch:
                    cases.append(("torch pad/gather/add " + label, n,
                                  lambda n=n, d_sh=d_sh: torch_sum(x, lo, hi, n, d_sh, out)))
        for c in cases:
            warm(c[2])
        times = {c[0]: [] for c in cases}
        for _ in range(a.rounds):
            for c in cases:
                times[c[0]].append(timed(c[2], a.iters))
        print("%-44s %9s %8s %8s | %7s %7s %7s | %7s %7s" % ("", "median ms", "min ms", "max ms", "1R+1W", "of 7.23", "of 6.24",
                                                             "nR+1W", "of 7.23"))
        for cname, n, _ in cases:
            t = sorted(times[cname])
            med = t[len(t) // 2]
            r1 = 8.0 * V * R * B / med
            rn = 4.0 * (n + 1) * V * R * B / med
            print("%-44s %9.3f %8.3f %8.3f | %7.3f %6.1f%% %6.1f%% | %7.3f %6.1f%%"
                  % (cname, med * 1e3, t[0] * 1e3, t[-1] * 1e3, r1 / 1e12, 100 * r1 / READ_CEILING, 100 * r1 / COPY_CEILING,
                     rn / 1e12, 100 * rn / READ_CEILING), flush=True)
        for integ in keep:
            integ.close()
        del x, out, cases, keep


def scr_line(a):
    import torch
    from rsp import inject, integrate, presets, score
    from rsp.engine import Engine
    spec = presets.dmx(128, 4096)
    rp = spec.radar
    B, n = 32, 4
    delta_r = rp.get("deltaR", 2.99792458e8 / (2 * rp.get("fs", 25e6)))
    v = 12.0
    dt = 2.0 * delta_r / v                                   # the CPIs of the dwell are dt apart: two cells per CPI
    Rg = 600.0 + v * dt * np.arange(B)
    plan = inject.target_plan(spec, Rg, np.full(B, v))
    truth = plan.truth_cells(spec, 0)
    assert (truth[:, 2] == 1).all()
    rows = (np.arange(spec.V) - spec.P // 2) * rp["wavelength"] / (2.0 * spec.P * rp["prt"])    # the velocity of each RDM row
    shift = integrate.walk_shifts(rows, dt, delta_r, n)
    rng = np.random.default_rng(4401)
    clutter = torch.from_numpy((rng.standard_normal((B, spec.P, spec.R)) + 1j * rng.standard_normal((B, spec.P, spec.R)))
                               .astype(np.complex64) * np.float32(0.7071)).to("cuda:0")
    scrs = [float(s) for s in np.arange(a.scr_lo, a.scr_hi + 0.5, a.scr_step)]
    cf = presets.default_cfar(spec)
    print("\nPd against SCR: %s, %d CPIs of one target at %.0f m/s, %.2f s between CPIs (%d cells per CPI, row %d), "
          "CFAR T = %g; the first n-1 CPIs of the dwell are part of the average"
          % (spec.name, B, v, dt, int(shift[0, truth[0, 0]]), int(truth[0, 0]), cf.TR), flush=True)
    with Engine(spec, device=0) as eng:
        integ = integrate.Integrator(engine=eng, n=n)
        lines = [("single CPI", score.scr_sweep(eng, clutter, plan, scrs, cf)),
                 ("n = 4, no walk", score.scr_sweep(eng, clutter, plan, scrs, cf, detector=integrate.detector(integ))),
                 ("n = 4, walk", score.scr_sweep(eng, clutter, plan, scrs, cf, detector=integrate.detector(integ, shift=shift)))]
    print("%-16s " % "SCR [dB]" + " ".join("%6.0f" % s for s in scrs))
    for name, res in lines:
        print("%-16s " % (name + " Pd") + " ".join("%6.3f" % r["drate"] for r in res))
    for name, res in lines:
        print("%-16s " % (name + " fa") + " ".join("%6.1f" % float(np.mean(r["fa"])) for r in res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the batches (a quick look: 0.25)")
    ap.add_argument("--scr", action="store_true", help="also the Pd-versus-SCR line")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--no-torch", action="store_true", help="the kernel's variants only (an A/B of two libraries)")
    ap.add_argument("--scr-lo", type=float, default=-44.0)
    ap.add_argument("--scr-hi", type=float, default=-20.0)
    ap.add_argument("--scr-step", type=float, default=2.0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("integ_bench: needs a GPU")
    if not a.no_bench:
        bench(a)
    if a.scr:
        scr_line(a)


if __name__ == "__main__":
    main()
