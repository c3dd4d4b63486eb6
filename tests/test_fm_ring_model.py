"""Host model of the value ring of the feature-major rectification scorers
(CPU suite).

``tests/cpp/fm_ring_model.cpp`` drives the ring allocator and the two wait
thresholds of ``csrc/fm_groups.h`` -- the functions k_score_fm itself calls --
first alone (one wave, fixed and random block sizes, random consumption
orders), then with 14 compute waves, the chain wave and the look-ahead wave as
host threads under ThreadSanitizer, with std::atomic counters for the LDS
flags.  It fails when a block leaves the ring or overlaps a published,
unfolded one, when a wave would wait for a round it has not published, when a
run-length row is rewritten before its round is folded, when a wave enters a
group two ahead of the written outputs, when a group does not complete (a
watchdog prints the counters), and -- rings and rows being plain memory --
when ThreadSanitizer sees an access the counters do not order.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "graph-cut-ransac_amd", "csrc")
SRC = os.path.join(HERE, "cpp", "fm_ring_model.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fm_ring") / "fm_ring_model_tsan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fno-omit-frame-pointer", "-fsanitize=thread",
                        "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "build failed:\n" + r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_allocator_invariants(model, seed):
    r = subprocess.run([model, "alloc", str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-6000:]
    assert r.stdout.count("OK alloc") == 2, r.stdout          # both depths: 4 (fused) and 2 (unfused)


@pytest.mark.parametrize("depth", [4, 2])
@pytest.mark.parametrize("mode", ["typical", "full", "empty"])
@pytest.mark.parametrize("rounds", [2, 3, 12])
def test_ring_hand_over(model, rounds, mode, depth):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([model, "threads", str(rounds), "8", mode, str(11 + rounds), "3", str(depth)],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-6000:]
    assert r.stdout.startswith("OK"), r.stdout
