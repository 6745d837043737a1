"""The fp16 screen's bytes (csrc/prune_screen_h2.hpp screen_h2_prep_kernel + prune_screen_h2_kernel) against recorded ones.

tests/golden/screen_h2_bytes_*.npz hold inputs and the four arrays tests/prune_screen_h2_driver.hip forms from the kernels'
output (mu_s, W, E, the closed form; 1 and 3 splits), recorded by tests/golden/make_golden_screen_h2_bytes.py from commit
8f33bde ("Pruned sweep: own header, named steps, one spelling of each launch"), before the screen's k loop lost its
accumulator zeroing and the prep kernel's row walk was interleaved.  A change of the kernels' instruction stream that is meant
to keep the arithmetic must keep these bytes."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_screen_h2_bytes as golden          # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "screen_h2_bytes_*.npz")))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prune_screen_h2_bytes") / "prune_screen_h2_driver")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", os.path.join(HERE, "prune_screen_h2_driver.hip"),
                           "-o", exe], timeout=900)
    return exe


def test_every_recorded_case_is_here():
    want = {"screen_h2_bytes_n%d_m%d_d%d.npz" % c for c in golden.CASES}
    assert {os.path.basename(f) for f in FIXTURES} == want


@pytest.mark.parametrize("splits", golden.SPLITS)
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[len("screen_h2_bytes_"):-len(".npz")])
def test_screen_writes_the_recorded_bytes(driver, tmp_path, path, splits):
    z = np.load(path)
    out = golden.run_driver(driver, splits, z["Xs"], z["Cs"], z["alpha"], float(z["constant"]), int(z["D"]), str(tmp_path))
    names = ("mu_s", "W", "E", "closed form")
    want = z["out_s%d" % splits]
    assert out[:4].tobytes() == out[4:8].tobytes()                      # the second run's bytes
    for k, name in enumerate(names):
        diff = int((out[k].view(np.uint64) != want[k].view(np.uint64)).sum())
        assert diff == 0, "%s: %d of %d values differ from the recorded bytes" % (name, diff, want.shape[1])
