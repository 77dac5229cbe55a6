"""The host-buffer entry points' planning arithmetic (radar-signal-process_amd/csrc/rsp_hostplan.h:
ring pieces, host chunks, the one-chunk path's input pieces and output parts) on the CPU, as a
stand-alone program: every element is delivered exactly once, pieces stay inside a plane and keep
their kernels' alignments, the parts fit the kParts events, and the default plans of known calls
are pinned.  The same program under AddressSanitizer + UBSan when the toolchain has them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "hostplan_check.cpp")
INC = os.path.join(ROOT, "radar-signal-process_amd", "csrc")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC, SRC, "-o", exe] + extra, check=True,
                   capture_output=True, text=True, timeout=300)
    return exe


def test_host_plan_properties(tmp_path):
    exe = _build(tmp_path, "hostplan_check", [])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_host_plan_under_sanitizers(tmp_path):
    try:
        exe = _build(tmp_path, "hostplan_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    except subprocess.CalledProcessError as e:
        pytest.skip("no ASan/UBSan in this toolchain: %s" % e.stderr[-300:])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-3000:]
