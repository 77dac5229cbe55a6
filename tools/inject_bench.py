#!/usr/bin/env python3
"""Target injection throughput at the c3 shape (1024 CPIs x 128 pulses x 4096 range bins,
complex64), four things timed in one process with HIP events, each after a 0.3 s warm-up, in
alternating rounds so that the spread between rounds is seen next to the differences:

  1. rsp_inject_dev   the point-target form: 8 B read + 8 B written per sample
  2. rsp_scr_dev      the general form with the clutter add: 16 B read + 8 B written
  3. rsp_prefilter_dev, gain only: the yardstick stream of the same bytes as (1)
  4. the injection of (1) written as a torch composition (per-segment power, gain, outer
     product with the target's row, add), which is what a user would write without (1); the
     target's row template and P_s are prepared outside the timed region

Rates are the bytes the algorithm needs (computed from the shape) over the event time, also as
a fraction of the 6.24 TB/s copy ceiling measured by tools/micro/hbm_ceiling.hip.
"""
import argparse
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
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()
        n += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--P", type=int, default=128)
    ap.add_argument("--R", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-target", action="store_true",
                    help="ranges in front of every segment: no CPI has a target, (1) reads no waveform")
    a = ap.parse_args()
    import numpy as np
    import torch
    from rsp import inject, prefilter, presets, synth
    if not torch.cuda.is_available():
        sys.exit("inject_bench: needs a GPU")
    B, P, R = a.batch, a.P, a.R
    spec = presets.v2(P, R)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    # one truth per CPI inside the gate, so every CPI has a target in the 200-sample MF segment
    rng_m = rng.uniform(450.0, 1900.0, B) - (1e4 if a.no_target else 0.0)
    plan = inject.target_plan(spec, rng_m, rng.uniform(4.0, 19.0, B) * rng.choice([-1, 1], B), device=dev)
    clutter = synth.echo_torch(spec, B, seed=5, device=dev)
    out = torch.empty_like(clutter)
    scr = torch.full((B,), 5.0, dtype=torch.float64, device=dev)
    inj = inject.Injector(0)
    pf = prefilter.Prefilter(0)
    gain = torch.full((R,), 1.25, dtype=torch.float32, device=dev)

    # the target's row per CPI and P_s per (CPI, segment), for (2) and (4)
    tmpl = torch.zeros((B, R), dtype=torch.complex64, device=dev)
    for s, (st, n) in enumerate(plan.segments):
        w = torch.from_numpy(plan.wf_host[s]).to(dev)
        for b in range(B):
            d = int(plan.delay[b, s])
            if d >= 0:
                k = min(len(w), n - d)
                tmpl[b, st + d:st + d + k] = w[:k]
    m = torch.arange(P, dtype=torch.float64, device=dev)
    phase = torch.polar(torch.ones((B, P), dtype=torch.float64, device=dev), plan.dphi_dev[:, None] * m[None, :])
    ps = [tmpl[:, st:st + n].abs().double().square().mean(-1) + 2.0 ** -52 for st, n in plan.segments]
    simu = (phase[:, :, None] * tmpl[:, None, :]).to(torch.complex64)
    out4 = torch.empty_like(clutter)

    def run_inject():
        inj.inject_dev(clutter, plan, scr, out=out)

    def run_scr():
        inj.scr_dev(simu, clutter, scr, plan.segments, seg_db=plan.seg_db, out=out)

    def run_prefilter():
        pf.apply_dev(clutter, out=out, gain=gain)

    def run_torch():
        out4.copy_(clutter)
        for s, (st, n) in enumerate(plan.segments):
            c = clutter[:, :, st:st + n]
            pe = (c.real.double().square() + c.imag.double().square()).mean(-1)
            g = torch.sqrt(pe * (10.0 ** ((scr + plan.seg_db[s]) / 10.0))[:, None] / ps[s][:, None])
            out4[:, :, st:st + n] += (g * phase).to(torch.complex64)[:, :, None] * tmpl[:, None, st:st + n]

    cases = [("1 rsp_inject_dev (point target)", run_inject, 16),
             ("2 rsp_scr_dev (general, add)", run_scr, 24),
             ("3 rsp_prefilter_dev (gain only)", run_prefilter, 16),
             ("4 torch composition of 1", run_torch, 16)]
    for name, fn, _ in cases:
        warm(fn)
    # like for like: (4) and (2) compute what (1) computes
    run_inject()
    ref = out[:2].clone()
    run_torch()
    run_scr()
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    print("shape %d x %d x %d complex64 (%.2f GB per buffer); check on 2 CPIs: torch vs inject %.2e, scr vs inject %.2e"
          % (B, P, R, B * P * R * 8 / 1e9, float((out4[:2] - ref).abs().max()) / scale,
             float((out[:2] - ref).abs().max()) / scale), flush=True)
    times = {name: [] for name, _, _ in cases}
    for _ in range(a.rounds):
        for name, fn, _ in cases:
            times[name].append(timed(fn, a.iters))
    samples = B * P * R
    print("%-34s %10s %10s %10s %9s %9s" % ("", "median ms", "min ms", "max ms", "TB/s", "of 6.24"))
    med = {}
    for name, _, bps in cases:
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        rate = samples * bps / med[name]
        print("%-34s %10.3f %10.3f %10.3f %9.3f %8.1f%%" % (name, med[name] * 1e3, t[0] * 1e3, t[-1] * 1e3, rate / 1e12,
                                                            100.0 * rate / CEILING), flush=True)
    n1, n3, n4 = cases[0][0], cases[2][0], cases[3][0]
    t3 = times[n3]
    print("inject / prefilter time %.3f (prefilter's own spread max/min %.3f); torch / inject %.2fx"
          % (med[n1] / med[n3], max(t3) / min(t3), med[n4] / med[n1]), flush=True)


if __name__ == "__main__":
    main()
