"""The pulse-compression launcher's long-row workgroup count
(radar-signal-process_amd/csrc/rsp_pcplan.h: pc_blocks, used by launch_pc_mf_n) on the CPU, as a
stand-alone program: u2 in {0, 1, 2, 3, 4, 5, 2048} units at 1, 2 and 4 rows per workgroup slot
against counts worked out by hand, and that the slots cover every unit with no empty workgroup."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pcplan_check.cpp")
INC = os.path.join(ROOT, "radar-signal-process_amd", "csrc")


def test_pc_block_counts(tmp_path):
    exe = str(tmp_path / "pcplan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC, SRC, "-o", exe], check=True,
                   capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
