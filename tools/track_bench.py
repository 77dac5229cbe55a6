#!/usr/bin/env python3
"""Tracking stage throughput (rsp_track_dev): batch 256, four slots (64 CPIs each,
interleaved), max_tracks 256, at about 64 and about 1000 valid plots per CPI.

The scene is synthetic and seeded: per slot constant-velocity targets seen with probability 0.9
under uniform false alarms over 3000 m x +-60 m/s, as tests/track_ref.py makes them.  Every timed
call starts from the same saved state (the tables after one pass over the batch, so they are as
full as they get), restored by a device copy inside the timed region of both variants' GPU side.

  1. rsp_track_dev on est / count resident on the device, snapshots written (HIP events; each
     variant after a warm-up of at least 3 calls and 0.3 s, in alternating rounds)
  2. the same work done by copying est and count to the host and running tests/track_ref.py there
     (host clock around the copy and the loop; once per round, it takes seconds)
  3. for scale, rsp_motion_measure_dev on the README's measure shape (2048 x 512, batch 256,
     about 1044 hits per CPI) on the same box

This stage is latency-bound: one workgroup per slot, four barriers per matching round.  The table
reports ms per batch and CPI/s, not a share of any peak.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "radar-signal-process_amd"), os.path.join(ROOT, "tests")]


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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--host-rounds", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch
    import track_ref as tr
    from rsp.measure import Measure
    from rsp.track import Tracker
    if not torch.cuda.is_available():
        sys.exit("track_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    B, S, T = a.batch, a.slots, 256
    per = B // S
    for name, targets, fa, H, gate in (("~64 plots", 8, 57, 128, (30.0, 2.0)), ("~1000 plots", 40, 964, 1024, (30.0, 2.0))):
        p = tr.Params(max_tracks=T, confirm=(3, 5), drop=(2, 4), dt=0.08, gate=gate, alpha=(0.5, 0.5, 0.5))
        est = np.full((B, H, 3), np.nan)
        count = np.zeros((B, 2), np.int32)
        slot = (np.arange(B) % S).astype(np.int32)
        for s in range(S):
            e, c, _ = tr.scene(9000 + s, cpis=per, targets=targets, false_alarms=fa, max_hits=H, dt=p.dt)
            est[s::S], count[s::S] = e, c
        d_est, d_count = torch.from_numpy(est).to(dev), torch.from_numpy(count).to(dev)
        d_slot = torch.from_numpy(slot).to(dev)
        trk = Tracker(0, slots=S, **p.kwargs())
        trk.update_dev(d_est, d_count, slot=d_slot)
        torch.cuda.synchronize()
        saved = trk.state()
        host_saved = tuple(t.cpu().numpy() for t in saved)

        def run_gpu():
            trk.load_state(saved)
            return trk.update_dev(d_est, d_count, slot=d_slot)

        def run_host():
            t0 = time.perf_counter()
            e, c = d_est.cpu().numpy(), d_count.cpu().numpy()
            state = tuple(x.copy() for x in host_saved)
            out = tr.run(state, e, c, p, slot=slot)
            return time.perf_counter() - t0, out, state

        # like for like: the bytes are the restatement's
        got = tuple(t.cpu().numpy() for t in run_gpu())
        torch.cuda.synchronize()
        _, want, want_state = run_host()
        same = all(g.tobytes() == w.tobytes() for g, w in zip(got, want)) and \
            all(t.cpu().numpy().tobytes() == w.tobytes() for t, w in zip(trk.state(), want_state))
        warm(run_gpu)
        gpu, host = [], []
        for r in range(a.rounds):
            gpu.append(timed(run_gpu, a.iters))
            if r < a.host_rounds:
                host.append(run_host()[0])
        gpu.sort()
        host.sort()
        tc = want[3]
        print("\n%s: batch %d on %d slots, max_tracks %d, max_hits %d; valid plots per CPI %.0f (mean), live entries %.0f "
              "(mean) / %d (max), matched %.0f per CPI; bytes equal to the restatement: %s"
              % (name, B, S, T, H, tc[:, tr.N_VALID].mean(), tc[:, tr.LIVE].mean(), tc[:, tr.LIVE].max(),
                 tc[:, tr.MATCHED].mean(), same), flush=True)
        print("%-44s %10s %10s %10s %12s" % ("", "median ms", "min ms", "max ms", "CPI/s"))
        g, h = gpu[len(gpu) // 2], host[len(host) // 2]
        print("%-44s %10.3f %10.3f %10.3f %12.0f" % ("1 rsp_track_dev (state restore included)", g * 1e3, gpu[0] * 1e3,
                                                      gpu[-1] * 1e3, B / g))
        print("%-44s %10.1f %10.1f %10.1f %12.0f" % ("2 copy to the host + track_ref", h * 1e3, host[0] * 1e3,
                                                      host[-1] * 1e3, B / h))
        print("host / device: %.0fx" % (h / g), flush=True)
        trk.close()

    # for scale: the measurement on the README's measure shape
    V, R, hits = 2048, 512, 1044
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    sum_rdm = torch.rand((B, V, R), generator=g, device=dev) + 1.0
    diff_rdm = torch.rand((B, V, R), generator=g, device=dev)
    flag = torch.zeros((B, V, R), dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(11)
    for b in range(B):
        v = torch.as_tensor(rng.integers(40, V - 40, hits), device=dev)
        r = torch.as_tensor(rng.integers(8, R - 8, hits), device=dev)
        flag[b, v, r] = 1
    meas = Measure(0)
    mp = meas.params(2, 7.5, 8, 0.3, 4, 1.0, 4, 5.0, 0.0, 0.0, 6)
    rs, vs = np.arange(R) * 7.5, np.arange(V) * 0.3   # host axes, uploaded by every call as the DMX loop's are

    def run_meas():
        meas.measure_dev(sum_rdm, diff_rdm, flag, mp, rs, vs, max_hits=2048)

    warm(run_meas)
    t = sorted(timed(run_meas, a.iters) for _ in range(a.rounds))
    print("\nfor scale, rsp_motion_measure_dev %d x %d, batch %d, %d hits per CPI: median %.3f ms (min %.3f, max %.3f), "
          "%.0f CPI/s" % (V, R, B, hits, t[len(t) // 2] * 1e3, t[0] * 1e3, t[-1] * 1e3, B / t[len(t) // 2]))
    meas.close()


if __name__ == "__main__":
    main()
