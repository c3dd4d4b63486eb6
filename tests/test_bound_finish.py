"""The rounding guard of verify_batches' bound path (csrc/bound.h): where
guard_holds() lets the path run, no finished score exceeds its slot's inlier
count by the margin of 1 the contender rule relies on.  tests/cpp/
bound_finish.cpp, a stand-alone host program built with ASan + UBSan."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "graph-cut-ransac_amd", "csrc")


def test_finish_stays_within_the_guard(tmp_path):
    exe = str(tmp_path / "bound_finish")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                           "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "bound_finish.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stdout.startswith("OK"), out.stdout
