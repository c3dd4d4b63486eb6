"""Host model of the grouped fused scorer's wave hand-over under
ThreadSanitizer (CPU suite).

``tests/cpp/fm_groups_model.cpp`` plays the 16 waves of one workgroup of
k_score_fm<KIND, 16, true> as host threads: 14 compute waves, the chain wave
and the look-ahead wave, with std::atomic counters for the LDS flags and the
index functions of ``csrc/fm_groups.h`` that the kernel itself uses (global
round, set parity, wait targets).  It fails when a survivor region is
rewritten before the chain wave has folded it, when a constant set is
rewritten while a wave of its group can still read it, when a group does not
complete (a watchdog prints the counters), and -- the regions, run lengths and
sets being plain memory -- when ThreadSanitizer sees an access the counters do
not order.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "graph-cut-ransac_amd", "csrc")
SRC = os.path.join(HERE, "cpp", "fm_groups_model.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fm_groups") / "fm_groups_model_tsan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fno-omit-frame-pointer", "-fsanitize=thread",
                        "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "build failed:\n" + r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("stage", ["a", "b"])
@pytest.mark.parametrize("groups", [1, 2, 3, 8])
@pytest.mark.parametrize("rounds", [1, 2, 3, 12])
def test_hand_over_across_groups(model, rounds, groups, stage):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([model, str(rounds), str(groups), stage, str(7 + rounds * 16 + groups), "3"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-6000:]
    assert r.stdout.startswith("OK"), r.stdout


def test_model_catches_an_early_set_rewrite(model, tmp_path):
    # canary: with the look-ahead wave's wait weakened by one group
    # (-DFMG_MODEL_EARLY_SET) the model must fail -- by its own tags or by a
    # ThreadSanitizer report -- so a pass above means something
    exe = str(tmp_path / "fm_groups_model_early")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fno-omit-frame-pointer", "-fsanitize=thread",
                        "-DFMG_MODEL_EARLY_SET", "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, "build failed:\n" + r.stderr[-4000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    caught = False
    for seed in range(1, 6):
        r = subprocess.run([exe, "3", "8", "b", str(seed), "3"], capture_output=True, text=True, timeout=120, env=env)
        if r.returncode != 0 and ("FAIL" in r.stderr or "ThreadSanitizer" in r.stderr):
            caught = True
            break
    assert caught, "the weakened hand-over ran clean: the model no longer exercises the set reuse"
