#!/usr/bin/env python3
"""Clutter-map stage throughput (rsp_cmap_dev) on pulse-compressed rows resident
in HBM, each batch well over the 256 MB cache:

  c3   128 x 4096, K = 3 (the MTD's /150 band) and K = 13 (main_cfar's /20 band), batch 256 (1 GiB)
  c5   512 x 16384, K = 53 (its /20 band), batch 16 (1 GiB)
  dmx  1536 pulses -> V 2048, two beams, 574 columns, K = 13 (zero_ends 7), batch 96 (1.3 GiB)

Timed in one process with HIP events, each variant after a warm-up of at least 3 calls and 0.3 s,
in alternating rounds so that the spread between rounds is seen next to the differences:

  1. rsp_cmap_dev (band + update + ages; the band amplitudes returned)
  2. rsp_mtd_cfar_dev on the same rows with the preset's default CFAR (the kernel that computes
     every Doppler row, of which the stage computes K)
  3. the stage as a torch composition (table product by einsum, the recursion a loop over the
     CPIs; a smaller batch, time scaled per CPI)

Rates: the PC rows' bytes over the whole call's event time -- a lower bound of the band kernel's
read rate, the update and age kernels run inside it -- also as a share of the 7.23 TB/s read
ceiling (profiles/hbm_ceiling.json).
"""
import argparse
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


def torch_stage(pc, tab, m, age, T, w, warmup, hold):
    """pc [B, beams, P, R] complex64, tab [K, P] complex64 -> (band, flag); m, age updated in place."""
    import torch
    band = torch.einsum("kp,bnpr->bnkr", tab, pc).abs().sum(1)
    flag = torch.zeros(band.shape, dtype=torch.uint8, device=pc.device)
    for b in range(band.shape[0]):
        a = band[b]
        if age == 0:
            m.copy_(a)
        else:
            f = (a >= T * m) if age >= max(warmup, 1) else torch.zeros_like(a, dtype=torch.bool)
            upd = m + w * (a - m)
            m.copy_(torch.where(f, m, upd) if hold else upd)
            flag[b] = f
        age += 1
    return band, flag, age


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-batch", type=int, default=4)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from rsp import presets
    from rsp.cmap import ClutterMap, band_of
    from rsp.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("cmap_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    T, w, warmup = 4.0, 0.125, 4
    shapes = [("c3 K=3", presets.dmx(128, 4096), False, 256), ("c3 K=13", presets.dmx(128, 4096), True, 256),
              ("c5 K=53", presets.dmx(512, 16384), True, 16), ("dmx K=13", presets.dmx_native(), True, 96)]
    for name, spec, wide, B in shapes:
        if a.only and a.only not in name:
            continue
        cfar = presets.default_cfar(spec)
        q_lo, q_hi = band_of(spec, cfar if wide else None)
        R, P, V, nb = spec.R_out, spec.P, spec.V, spec.beams
        g = torch.Generator(device=dev)
        g.manual_seed(4100)
        shape = (B, P, R) if nb == 1 else (B, nb, P, R)
        pc = torch.view_as_complex(torch.randn(shape + (2,), generator=g, device=dev))
        pc[..., ::3] += 30.0
        cm = ClutterMap(spec, band=(q_lo, q_hi), T=T, w=w, warmup=warmup, hold=True)
        plan = cm.plan(B)
        eng = Engine(spec)
        rdm = torch.empty((B, V, R), dtype=torch.float32, device=dev)
        flag = torch.empty((B, V, R), dtype=torch.uint8, device=dev)
        tb = min(a.torch_batch, B)
        k = torch.arange(q_lo, q_hi + 1, dtype=torch.float64)[:, None]
        p = torch.arange(P, dtype=torch.float64)[None, :]
        win = {0: lambda: torch.as_tensor(presets.kaiser(P, spec.window_beta)), 1: lambda: torch.hamming_window(
            P, periodic=False, dtype=torch.float64), 2: lambda: torch.ones(P, dtype=torch.float64)}[spec.window]()
        tab = (win[None, :] * torch.exp(-2j * np.pi * ((k * p) % V) / V)).to(torch.complex64).to(dev)
        pct = pc[:tb].reshape(tb, nb, P, R)
        tm = torch.zeros((cm.K, R), device=dev)

        def run_cmap():
            cm.update_dev(pc)

        def run_mtd():
            eng.mtd_dev(pc, rdm=rdm, flag=flag, cfar=cfar)

        def run_torch():
            torch_stage(pct, tab, tm, 1, T, w, warmup, True)

        cases = [("1 rsp_cmap_dev", run_cmap, B), ("2 rsp_mtd_cfar_dev (all %d rows)" % V, run_mtd, B),
                 ("3 torch composition of 1 (batch %d)" % tb, run_torch, tb)]
        # like for like: the torch composition computes the same amplitudes
        cm.reset()
        band, _ = cm.update_dev(pc[:tb].contiguous())
        tband, _, _ = torch_stage(pct, tab, tm, 0, T, w, warmup, True)
        torch.cuda.synchronize()
        err = float((band - tband).norm() / tband.norm())
        for _, fn, _ in cases:
            warm(fn)
        nbytes = B * nb * P * R * 8
        print("\n%s: %d CPIs of %d beam(s) x %d x %d (%.2f GiB of PC rows), bins %d..%d; plan %s; band against torch: rel %.2g"
              % (name, B, nb, P, R, nbytes / 2.0 ** 30, q_lo, q_hi,
                 {n: plan[n] for n in ("bins_per_pass", "passes", "vec", "split")}, err), flush=True)
        times = {n: [] for n, _, _ in cases}
        for _ in range(a.rounds):
            for n, fn, _ in cases:
                times[n].append(timed(fn, a.iters if "torch" not in n else 1))
        print("%-38s %10s %10s %10s %12s %9s %8s" % ("", "median ms", "min ms", "max ms", "CPI/s", "PC TB/s", "of 7.23"))
        med = {}
        for n, _, cb in cases:
            t = sorted(times[n])
            med[n] = t[len(t) // 2] / cb
            rate = nbytes / B / med[n]
            share = "%9.3f %7.1f%%" % (rate / 1e12, 100.0 * rate / CEILING) if n[0] == "1" else ""
            print("%-38s %10.3f %10.3f %10.3f %12.0f %s" % (n, t[len(t) // 2] * 1e3, t[0] * 1e3, t[-1] * 1e3,
                                                         1.0 / med[n], share), flush=True)
        n1, n2, n3 = (c[0] for c in cases)
        print("rsp_cmap_dev / rsp_mtd_cfar_dev: %.2fx the time (the stage computes %d of %d rows); torch / rsp_cmap_dev "
              "per CPI: %.1fx" % (med[n1] / med[n2], cm.K, V, med[n3] / med[n1]), flush=True)
        cm.close()
        eng.close()
        del pc, rdm, flag, pct
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
