#!/usr/bin/env python3
"""Times rsp_score_dev (csrc/rsp_score.hip) on a device-resident c3-sized batch.

The flags and the RDM come from the chain itself (Engine.run_dev on synthetic echoes, default
CFAR); every second truth is valid and sits on an injected target, so its CPI has a flag in
the fun_PCF box and its RDM is scanned for the peak -- the dearest case for a valid truth.
HIP events around each call after a 0.3 s warm-up, median of --runs calls.  Reported:
microseconds per step, the bytes the pass reads (all flag bytes, plus the RDM of the CPIs that
scan it, counted from the records), the fraction of the measured HBM read ceiling
(profiles/hbm_ceiling.json) and the ratio to the chain's own step time, measured the same way
in this process (or given with --chain-ms, e.g. bench.py's ms_per_step on the same box).

    python tools/score_probe.py [--batch 1024 --P 128 --R 4096] [--out profiles/score_probe.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "radar-signal-process_amd")]


def timed(torch, fn, runs, warm_s=0.3):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        fn()
        torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--P", type=int, default=128)
    ap.add_argument("--R", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--chain-ms", type=float, default=None, help="the chain's step time from bench.py on the same box")
    ap.add_argument("--small", action="store_true", help="also time batches of 1, 4 and 16 CPIs")
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    args = ap.parse_args()

    import numpy as np
    import torch
    from rsp import presets, score, synth
    from rsp.engine import Engine

    if not torch.cuda.is_available():
        sys.exit("score_probe: needs a GPU (a CPU run measures nothing)")
    spec = presets.v2(args.P, args.R)
    cfar = presets.default_cfar(spec)
    eng = Engine(spec, device=0)
    B, V, R = args.batch, spec.V, spec.R_out
    echo = synth.echo_torch(spec, B, seed=1000, device="cuda:0")
    rdm = torch.empty((B, V, R), dtype=torch.float32, device="cuda:0")
    flag = torch.empty((B, V, R), dtype=torch.uint8, device="cuda:0")

    def chain():
        eng.run_dev(echo, rdm=rdm, flag=flag, cfar=cfar)

    chain_ms = timed(torch, chain, max(5, args.runs // 3))
    # truths: the second target of synth (a matched-filter segment), valid for every other CPI
    rp = spec.radar
    _, d, v = synth._targets(spec)[1]
    row = int(round(2 * v / rp["wavelength"] * spec.P * rp["prt"])) + spec.P // 2
    truth = np.tile(np.array([[row, d, 1]], np.int32), (B, 1))
    truth[1::2, 2] = 0
    truth_dev = torch.from_numpy(truth).to("cuda:0")
    params = score.score_params(v_lim=V, r_lim=R)
    sc = score.Scorer(engine=eng)

    def run(n=B, with_rdm=True):
        return sc.score_dev(flag[:n], rdm[:n] if with_rdm else None, truth_dev[:n], params)

    rec = run().cpu().numpy()
    assert (rec[:, 0] == flag.view(B, -1).sum(1, dtype=torch.int64).cpu().numpy()).all(), "n_flags differs from flag.sum()"
    scanned = int((rec[:, 5] > 0).sum())
    med, lo, hi = timed(torch, run, args.runs)
    med_f, _, _ = timed(torch, lambda: run(with_rdm=False), args.runs)
    ceiling = json.load(open(os.path.join(ROOT, "profiles", "hbm_ceiling.json")))["read_GBps"]
    nbytes = B * V * R + scanned * V * R * 4
    ref_ms = args.chain_ms if args.chain_ms is not None else chain_ms[0]
    out = {
        "what": "rsp_score_dev on a device-resident batch from run_dev (HIP events, median of %d after 0.3 s warm-up)" % args.runs,
        "shape": {"batch": B, "V": V, "R": R},
        "valid_truths": int(truth[:, 2].sum()), "cpis_scanning_rdm": scanned,
        "detected": int(((rec[:, 1] > 0) & (truth[:, 2] != 0)).sum()),
        "us_per_step": round(med * 1e3, 1), "us_min": round(lo * 1e3, 1), "us_max": round(hi * 1e3, 1),
        "bytes_read_per_step": nbytes,
        "GBps": round(nbytes / (med * 1e-3) / 1e9, 1),
        "read_ceiling_GBps": ceiling,
        "fraction_of_read_ceiling": round(nbytes / (med * 1e-3) / 1e9 / ceiling, 3),
        "flags_only": {"us_per_step": round(med_f * 1e3, 1), "bytes": B * V * R,
                       "GBps": round(B * V * R / (med_f * 1e-3) / 1e9, 1),
                       "fraction_of_read_ceiling": round(B * V * R / (med_f * 1e-3) / 1e9 / ceiling, 3)},
        "chain_ms_per_step": round(ref_ms, 4),
        "chain_ms_source": "bench.py (--chain-ms)" if args.chain_ms is not None else "run_dev timed in this process",
        "score_over_chain": round(med / ref_ms, 4),
    }
    if args.small:
        out["small_batches_us"] = {str(n): round(timed(torch, lambda n=n: run(n), args.runs)[0] * 1e3, 1) for n in (1, 4, 16)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
