#!/usr/bin/env python3
"""Legacy-record decode throughput: one file's worth per call (10 frames of 1536 PRTs x 1031
samples, 190.6 MB of records resident in HBM -> 253 MB of complex64 in two beam planes per
frame), two things timed in one process with HIP events, each after 0.3 s of warm-up (at least
3 calls, as bench.py warms), in alternating rounds so that the spread between rounds is seen
next to the difference:

  1. rsp_ingest_legacy_dev   one launch: 12 B read + 16 B written per sample, plus the head
                             fields, angle and status per PRT
  2. the same decode written as a torch composition (uint8 slicing, integer shifts, where,
     conversion, strided stores into the same output), which is what a user would write
     without (1)

Rates are the bytes the decode has to move, computed from the shape (rec_bytes * rows read;
16 * rows * point_prt + (8 + 32 + 4) * rows + 4 written), over the event time, also as a fraction
of the copy ceiling in profiles/hbm_ceiling.json (tools/micro/hbm_ceiling.hip).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "radar-signal-process_amd")]


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
    while time.perf_counter() - t0 < seconds or n < 3:
        fn()
        torch.cuda.synchronize()
        n += 1
    return n


def synth_stream(rows, point, seed, device):
    """Random record bytes made on the device (every byte uniform: the full 24-bit range in every
    channel, arbitrary heads)."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    rec = 28 + 12 * point + 8
    return torch.randint(0, 256, (rows * rec,), dtype=torch.uint8, device=device, generator=g)


def torch_decode(stream, prt, point, nframes, out, angle, head):
    """frameDataRead_A's decode as torch ops on the device: out [F][2][P][R] complex64, angle
    float64 [F][P], head int32 [F][P][8]."""
    import torch
    rows = prt * nframes
    rec = 28 + 12 * point + 8
    r = stream.view(rows, rec)
    g = r[:, 28:28 + 12 * point].reshape(rows, point, 3, 4).to(torch.int32)
    v = (g[:, :, 0, :] << 16) | (g[:, :, 1, :] << 8) | g[:, :, 2, :]            # [rows][point][Ql Il Qr Ir]
    v = torch.where(v > (1 << 23), v - (1 << 24), v).to(torch.float32)
    o = torch.view_as_real(out).view(nframes, 2, prt, point, 2)
    v = v.view(nframes, prt, point, 4)
    o[:, 0, :, :, 0], o[:, 0, :, :, 1] = v[..., 1], v[..., 0]
    o[:, 1, :, :, 0], o[:, 1, :, :, 1] = v[..., 3], v[..., 2]
    h = r[:, :28].to(torch.int32)
    u16 = h[:, 0:16:2] | (h[:, 1:16:2] << 8)
    hd = head.view(rows, 8)
    fi = (u16[:, 2].to(torch.int64) << 16) | u16[:, 3].to(torch.int64)
    hd[:, 0] = torch.where(fi >= (1 << 31), fi - (1 << 32), fi)                 # the 32-bit pattern, as the kernel stores it
    hd[:, 1], hd[:, 2], hd[:, 3], hd[:, 4], hd[:, 5] = u16[:, 4], h[:, 10], h[:, 11], u16[:, 6], u16[:, 7]
    hd[:, 6] = ((u16[:, 0] == 0xA5A5) & (u16[:, 1] == 0xA5A5)).to(torch.int32)
    hd[:, 7] = 0
    angle.view(rows)[:] = ((h[:, 26] + (h[:, 27] << 7)) * 360).to(torch.float64) / 16384.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--prt", type=int, default=1536)
    ap.add_argument("--point", type=int, default=1031)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from rsp import ingest
    if not torch.cuda.is_available():
        sys.exit("legacy_ingest_bench: needs a GPU")
    with open(os.path.join(ROOT, "profiles", "hbm_ceiling.json")) as f:
        ceiling = json.load(f)["copy_GBps"] * 1e9
    F, P, R = a.frames, a.prt, a.point
    rows = F * P
    dev = torch.device("cuda", 0)
    ing = ingest.LegacyIngest(0)
    rec = ing.record_bytes(R)
    stream = synth_stream(rows, R, 1, dev)
    out = torch.empty((F, 2, P, R), dtype=torch.complex64, device=dev)
    out2 = torch.empty_like(out)
    angle2 = torch.empty((F, P), dtype=torch.float64, device=dev)
    head2 = torch.empty((F, P, 8), dtype=torch.int32, device=dev)
    res = {}

    def run_kernel():
        res["k"] = ing.decode_dev(stream, stream.numel(), P, R, F, out=out)

    def run_torch():
        torch_decode(stream, P, R, F, out2, angle2, head2)

    cases = [("1 rsp_ingest_legacy_dev", run_kernel), ("2 torch composition of 1", run_torch)]
    for _, fn in cases:
        warm(fn)
    # like for like: (2) computes what (1) computes, bit for bit
    run_kernel()
    run_torch()
    torch.cuda.synchronize()
    _, angle, head, status = res["k"]
    same = (torch.equal(torch.view_as_real(out), torch.view_as_real(out2)) and torch.equal(angle, angle2)
            and torch.equal(head, head2) and int(status[rows]) == rows and not bool(status[:rows].any()))
    bytes_in = rec * rows
    bytes_out = 16 * rows * R + (8 + 32 + 4) * rows + 4
    print("%d frames x %d PRTs x %d samples: %.1f MB of records -> %.1f MB out; torch == kernel bit for bit: %s"
          % (F, P, R, bytes_in / 1e6, bytes_out / 1e6, same), flush=True)
    if not same:
        sys.exit("legacy_ingest_bench: the torch composition and the kernel disagree")
    times = {name: [] for name, _ in cases}
    for _ in range(a.rounds):
        for name, fn in cases:
            times[name].append(timed(fn, a.iters))
    print("%-28s %10s %10s %10s %10s %9s %11s" % ("", "median ms", "min ms", "max ms", "frames/s", "TB/s", "of ceiling"))
    med = {}
    for name, _ in cases:
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        rate = (bytes_in + bytes_out) / med[name]
        print("%-28s %10.3f %10.3f %10.3f %10.0f %9.3f %10.1f%%" % (name, med[name] * 1e3, t[0] * 1e3, t[-1] * 1e3,
                                                                    F / med[name], rate / 1e12, 100.0 * rate / ceiling),
              flush=True)
    n1, n2 = cases[0][0], cases[1][0]
    t1 = times[n1]
    print("copy ceiling %.3f TB/s (profiles/hbm_ceiling.json); torch / kernel time %.2fx (kernel's own spread max/min %.3f)"
          % (ceiling / 1e12, med[n2] / med[n1], max(t1) / min(t1)), flush=True)
    ing.close()


if __name__ == "__main__":
    main()
