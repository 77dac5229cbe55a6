#!/usr/bin/env python3
"""Ordered-statistic CFAR throughput (rsp_os_cfar_dev) beside the cell-averaging
detector (rsp_cfar_dev) on the same planes, resident in HBM:

  c3         128 x 4096 planes, batch 256 (ld = R), M0 = 2
  dmx short  2048 x 62, the column window (0, 62) of ld = 574 planes, batch 96, M0 = 6
  dmx long   2048 x 512, the column window (62, 574) of the same planes

Amplitudes: Rayleigh noise of mean 1 plus 64 point targets of 40 per CPI.  Window ref 5 / guard 7,
T = 7 in both stages; the forms are union k = 7 and per-side greatest-of k = 4, each with rFlag 0
and 1.  rsp_cfar_dev (greatest-of the means, T = 7) takes dense planes only, so for the two windows
it runs on dense copies of the same columns.

Timed in one process with HIP events, every variant after a warm-up of at least 3 calls and 0.3 s,
in alternating rounds so that the spread between rounds is seen next to the differences.  Bytes
moved per cell: 4 read + flagV written + flag written with rFlag 0 (6 B), and the range stage's
read of flagV on top with rFlag 1 (7 B; its amplitude reads at the hits are not counted), over the
whole call's event time, also as a share of the 7.23 TB/s read ceiling (profiles/hbm_ceiling.json).
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


def planes(B, V, Rp, M0, seed, dev):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.view_as_complex(torch.randn((B, V, Rp, 2), generator=g, device=dev)).abs() * 0.7978845608   # mean 1
    n = 64
    b = torch.arange(B, device=dev).repeat_interleave(n)
    v = torch.randint(M0 + 1, V - M0, (B * n,), generator=g, device=dev)
    r = torch.randint(0, Rp, (B * n,), generator=g, device=dev)
    x[b, v, r] = 40.0
    return x.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the batches (a quick look: 0.25)")
    a = ap.parse_args()
    import torch
    from rsp import oscfar, presets
    if not torch.cuda.is_available():
        sys.exit("oscfar_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    oc = oscfar.OsCfar(0)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    T = 7.0
    shapes = []
    B3 = max(1, int(256 * a.scale))
    shapes.append(("c3 128x4096", planes(B3, 128, 4096, 2, 4300, dev), 0, 4096, 2))
    Bd = max(1, int(96 * a.scale))
    xd = planes(Bd, 2048, 574, 6, 4301, dev)
    shapes.append(("dmx short 2048x62", xd, 0, 62, 6))
    shapes.append(("dmx long 2048x512", xd, 62, 574, 6))
    print("window ref 5 / guard 7, T = %g; %d iterations x %d rounds per variant" % (T, a.iters, a.rounds), flush=True)
    for name, x, lo, hi, M0 in shapes:
        B, V, Rp = x.shape
        R = hi - lo
        dense = x if (lo, hi) == (0, Rp) else x[:, :, lo:hi].contiguous()
        flag = torch.empty((B, V, Rp), dtype=torch.uint8, device=dev)
        flagV = torch.empty((B, V, Rp), dtype=torch.uint8, device=dev)
        dflag = torch.empty((B, V, R), dtype=torch.uint8, device=dev)
        dflagV = torch.empty((B, V, R), dtype=torch.uint8, device=dev)
        cases = []

        def os_case(k, union, rflag):
            cp = presets.Cfar(refR=5, saveR=7, TR=T, refV=5, saveV=7, TV=T, M0=M0, rFlag=rflag, zero_v_div=0).to_c()
            op = oscfar.os_params((k, k), (union, union))
            op.ld, op.cpi_stride = Rp, V * Rp

            def run():
                rc = oc.lib.rsp_os_cfar_dev(oc.ctx, x.data_ptr() + 4 * lo, V, R, B, C.byref(cp), C.byref(op),
                                            flag.data_ptr() + lo, flagV.data_ptr() + lo, st)
                assert rc == 0, oc.lib.rsp_last_error(oc.ctx)
            return run

        def ca_case(rflag):
            cp = presets.Cfar(refR=5, saveR=7, TR=T, refV=5, saveV=7, TV=T, M0=M0, rFlag=rflag, zero_v_div=0).to_c()

            def run():
                rc = oc.lib.rsp_cfar_dev(oc.ctx, dense.data_ptr(), V, R, B, C.byref(cp), dflag.data_ptr(),
                                         dflagV.data_ptr(), st)
                assert rc == 0, oc.lib.rsp_last_error(oc.ctx)
            return run

        for rflag in (0, 1):
            for label, k, union in (("union k=7", 7, True), ("GO k=4", 4, False)):
                fn = os_case(k, union, rflag)
                fn()
                torch.cuda.synchronize()
                hits = float(flag[:, :, lo:hi].sum()) / B
                hitsV = float(flagV[:, :, lo:hi].sum()) / B
                cases.append(("rsp_os_cfar_dev %s rFlag %d" % (label, rflag), fn, 7 if rflag else 6, rflag, hits, hitsV))
            fn = ca_case(rflag)
            fn()
            torch.cuda.synchronize()
            cases.append(("rsp_cfar_dev GO means rFlag %d" % rflag, fn, 7 if rflag else 6, rflag,
                          float(dflag.sum()) / B, float(dflagV.sum()) / B))
        plan = oc.plan(V, R, B, presets.Cfar(refR=5, saveR=7, TR=T, refV=5, saveV=7, TV=T, M0=M0, zero_v_div=0), (7, 7),
                       (True, True))
        print("\n%s: %d CPIs, %d x %d window at column %d of ld = %d; Doppler tile 2^%d columns, %d range tile(s) per row"
              % (name, B, V, R, lo, Rp, plan["v_tile_log2"], plan["r_tiles"]), flush=True)
        for c in cases:
            warm(c[1])
        times = {c[0]: [] for c in cases}
        for _ in range(a.rounds):
            for c in cases:
                times[c[0]].append(timed(c[1], a.iters))
        print("%-36s %9s %8s %8s %9s %7s %8s %10s %10s" % ("", "median ms", "min ms", "max ms", "CPI/s", "TB/s",
                                                           "of 7.23", "flag/CPI", "flagV/CPI"))
        med = {}
        for cname, _, bpc, rflag, hits, hitsV in cases:
            t = sorted(times[cname])
            med[cname] = t[len(t) // 2]
            rate = float(bpc) * V * R * B / med[cname]
            print("%-36s %9.3f %8.3f %8.3f %9.0f %7.3f %7.1f%% %10.1f %10.1f"
                  % (cname, med[cname] * 1e3, t[0] * 1e3, t[-1] * 1e3, B / med[cname], rate / 1e12, 100.0 * rate / CEILING,
                     hits, hitsV), flush=True)
        for cname, _, _, rflag, _, _ in cases:
            if cname.startswith("rsp_os"):
                print("%s / rsp_cfar_dev: %.2fx the time" % (cname, med[cname] / med["rsp_cfar_dev GO means rFlag %d" % rflag]),
                      flush=True)
        del flag, flagV, dflag, dflagV, dense
    oc.close()


if __name__ == "__main__":
    main()
