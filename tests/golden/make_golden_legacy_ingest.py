#!/usr/bin/env python3
"""Generate tests/golden/legacy_ingest_3x20.npz: a small synthetic stream of the legacy two-beam
24-bit PRT records (tests/legacy_ingest_ref.synth_legacy_stream: 3 PRTs of 20 samples, one frame)
with its decode by the integer restatement of frameDataRead_A_xzr.m in the same module.  The
reference ships no .bin capture, so the input is synthetic (seeded); the file pins the
restatement over time and gives the GPU path a fixed target.

Run from the repo root:  python tests/golden/make_golden_legacy_ingest.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import legacy_ingest_ref as ref  # noqa: E402


def main():
    prt, point = 3, 20
    stream = ref.synth_legacy_stream(prt, point, 1, seed=2409)
    d = ref.decode_stream(stream, prt, point, 1)
    assert d["status"][prt] == prt
    np.savez_compressed(os.path.join(HERE, "legacy_ingest_3x20.npz"), stream=stream, left=d["left"][0], right=d["right"][0],
                        angle=d["angle"][0], head=d["head"][0])
    print("wrote legacy_ingest_3x20.npz (%d bytes of records)" % stream.size)


if __name__ == "__main__":
    main()
