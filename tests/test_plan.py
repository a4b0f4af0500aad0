"""CPU: subread_amd/csrc/svg_plan.h -- the per-read probe plan, the multiply-shift quotients and
the slot-major probe index of the line probe kernel -- checked exhaustively against the literal
division forms by a stand-alone program (tests/native/plan_check.cc), built with the system
compiler."""
import os
import subprocess

from tests.common import ROOT


def test_plan_matches_literal_arithmetic(tmp_path):
    exe = tmp_path / "plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", str(exe),
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "subread_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "plan_check.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # 192 gaps x 2 subread counts x 1212 lengths x 192 probes alone are 89,358,336 comparisons
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 89_358_336
