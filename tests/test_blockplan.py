"""CPU: subread_amd/csrc/svg_blockplan.h -- where a multi-block index splits, planned from the contig
layout and one question about the kept windows -- checked against the literal per-window walk of
the CPU builder by a stand-alone program (tests/native/blockplan_check.cc), built with the system
compiler: contig-start splits around a 17-base contig, deep splits with the 1,999,974 step back,
one-block plans, a budget landing on a contig's last window, the 100-block error and the handle
limit, gap 1 and 3, all-kept / random / run-structured bitmaps."""
import os
import subprocess

from tests.common import ROOT


def test_blockplan_matches_per_window_walk(tmp_path):
    exe = tmp_path / "blockplan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", str(exe),
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "subread_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "blockplan_check.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # 2 gaps x (28 synth + 10 deep + 12 lone + 24 last-window + 3 start-cycle) plans at the least,
    # each compared block by block and segment by segment
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 2000
