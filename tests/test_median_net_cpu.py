"""The 5x5 median's comparator network (csrc/rbf_median_net.h: 32-wire Batcher restricted to 25 wires, read at wire 12) is a median for
EVERY input, not only for the planes the GPU tests happen to draw: tests/c/median_net_cases.cpp, built with g++ -std=c++17 -- no HIP
compiler, which is the proof that the header pulls in no kernel header -- replays the list as median25 (csrc/rbf_kernels_noise.h) does and
walks all 2 x 5,200,300 inputs of 12 and of 13 ones.  No GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")
LAYER = 5200300                      # C(25, 12) = C(25, 13)


@pytest.fixture(scope="module")
def median_net_cases(tmp_path_factory):
    if GXX is None:
        pytest.skip("g++ not found: tests/c/median_net_cases.cpp is built with a plain host compiler, not with hipcc")
    exe = str(tmp_path_factory.mktemp("median_net") / "median_net_cases")
    r = subprocess.run([GXX, "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-Werror",
                        os.path.join(REPO, "tests", "c", "median_net_cases.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_median_network_is_a_median_for_every_input(median_net_cases):
    """A network of min/max is monotone in every input, so on 0/1 inputs: 0 for all inputs of 12 ones gives 0 for every input of <= 12
    ones, 1 for all of 13 ones gives 1 for every input of >= 13.  Wire 12 is then `ones >= 13` on all 2^25 0/1 inputs, and by the 0-1
    principle (min/max commute with every threshold `value >= t`) it is the 13th smallest of any 25 values.

    Measured: 140 comparators = 280 min/max of which 202 can reach wire 12 -- the 101 + 101 packed min/max in k_noise_moments' assembly."""
    out = subprocess.run([median_net_cases], capture_output=True, text=True)
    lines = out.stdout.split("\n")
    assert out.returncode == 0 and lines[-2:] == ["ok", ""], out.stdout[-2000:] + out.stderr[-2000:]
    got = dict(ln.split(None, 1) for ln in lines[:-2])
    assert got["ones12"] == str(LAYER) and got["ones13"] == str(LAYER), out.stdout
    assert got["comparators"] == "140" and got["operations"] == "280 live 202", out.stdout


@pytest.mark.parametrize("comparator,layer", [(0, 12), (50, 12), (100, 13)])
def test_the_proof_notices_a_missing_comparator(median_net_cases, comparator, layer):
    """The same walk with one comparator left out names an input of the layer that comparator serves: the proof can fail."""
    out = subprocess.run([median_net_cases, "drop", str(comparator)], capture_output=True, text=True)
    last = out.stdout.strip().split("\n")[-1]
    assert out.returncode == 1 and last.startswith("FAIL input=0x") and "ones=%d " % layer in last, out.stdout[-2000:]
    assert bin(int(last.split("input=")[1].split()[0], 16)).count("1") == layer
