"""The pruned sweep's shortened tail (csrc/trmm_sweep.hpp trmm_sumsq_glds_narrow_kernel, csrc/sweep_pruned.hpp
contract_variant / sweep_pruned).

* The narrow contraction (128 rows x 32 / 64 candidates, the four waves splitting the rows) against the 128 x 128 kernel
  on the same gathered rows: `part` and the mean compared byte for byte -- tests/prune_tail_driver.hip, compiled here
  against the library's own header, launches the three kernels side by side.
* Forced survivors (a small TGP_PRUNE_TOP, every survivor taken) through the pruned schedule: winner value and index equal
  to the unpruned sweep's bit for bit, ties between the lb set and a survivor included, `n_clamped` unchanged."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NS = (300, 1000, 4096)          # padding, edge tiles, the flagship size
ROWS = (1, 127, 128, 256, 1000)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prune_tail") / "prune_tail_driver")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", os.path.join(HERE, "prune_tail_driver.hip"),
                           "-o", exe], timeout=900)
    return exe


@pytest.fixture(scope="module")
def driver_lines(driver):
    """every (dtype, N, rows) case in one process per dtype: {(dtype, N, rows, bn): (part_diff, mu_diff, ref_ok)}"""
    out = {}
    for dtype in ("f32", "f64"):
        args = [driver, dtype]
        for n in NS:
            for r in ROWS:
                args += [str(n), str(r)]
        res = subprocess.run(args, capture_output=True, text=True, timeout=600)
        print(res.stdout)
        assert res.returncode in (0, 1), res.stdout[-2000:] + res.stderr[-2000:]
        for line in res.stdout.splitlines():
            f = line.split()
            kv = dict(x.split("=") for x in f[1:])
            out[(f[0], int(kv["N"]), int(kv["rows"]), int(kv["bn"]))] = (int(kv["part_diff"]), int(kv["mu_diff"]), int(kv["ref_ok"]))
    return out


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_narrow_contraction_writes_the_128_tile_kernels_bits(driver_lines, dtype, N, rows):
    for bn in (32, 64):
        part_diff, mu_diff, ref_ok = driver_lines[(dtype, N, rows, bn)]
        assert ref_ok == 1, "the 128 x 128 kernel's own output is empty"
        assert part_diff == 0 and mu_diff == 0, (dtype, N, rows, bn, part_diff, mu_diff)


@pytest.fixture(scope="module")
def forced(request):
    e = dict(os.environ)
    e.update(TGP_PRUNE_TOP="4", TGP_PRUNE_FRAC="1", TGP_PRUNE_MIN_WORK="0")
    out = subprocess.run([sys.executable, os.path.join(HERE, "_prune_tail_child.py")], env=e, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "prune-tail ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    recs = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    assert len(recs) == 4
    return recs


@pytest.mark.parametrize("i", range(4))
def test_forced_survivors_give_the_unpruned_winner(forced, i):
    r = forced[i]
    print(r)
    assert r["prune"]["state"] == 0 and r["prune"]["lb_set"] == 4 and r["prune"]["survivors"] > 0, r["prune"]
    assert r["prune_off"]["state"] == -1
    assert r["full"]["best_idx"] == r["argmax"]
    assert r["pruned"] == r["unpruned"] == r["full"], r
    if r["tie"]:
        # the lowest copy of the winner's row wins; it is the lb set's pick of its group or a survivor beside it
        assert r["full"]["best_idx"] == r["copies"][0], r
