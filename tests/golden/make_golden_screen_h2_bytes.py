"""Records tests/golden/screen_h2_bytes_*.npz: inputs of the fp16 screen and the four arrays tests/prune_screen_h2_driver.hip
forms from what screen_h2_prep_kernel + prune_screen_h2_kernel write (mu_s, W, E, the closed form), for 1 and 3 splits.

Needs a GPU and the driver built from the commit whose bytes are to be pinned:
    hipcc -O3 -std=c++17 --offload-arch=gfx950 tests/prune_screen_h2_driver.hip -o DRIVER
    python tests/golden/make_golden_screen_h2_bytes.py DRIVER [OUTDIR]
tests/test_gpu_prune_screen_h2_bytes.py asserts that the current build writes the same bytes."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# (N, M, D): one 32-k chunk; a ragged chunk (17 of 32 k, one 16-k block of zeros); two chunks with their own candidate
# staging (40 = 32 + 8); two full chunks and N = 129 -- a positive and a negative tile, the sign boundary inside split 0
CASES = ((300, 256, 32), (300, 256, 17), (257, 128, 40), (129, 128, 64))
SPLITS = (1, 3)


def make_inputs(N, M, D, seed):
    rng = np.random.RandomState(seed)
    Dp = -(-D // 4) * 4
    ls = 0.35 * np.sqrt(D)
    Xs = np.zeros((N, Dp), dtype=np.float32)
    Cs = np.zeros((M, Dp), dtype=np.float32)
    Xs[:, :D] = rng.uniform(0, 1, size=(N, D)) / ls
    Cs[:, :D] = rng.uniform(0, 1, size=(M, D)) / ls
    Cs[::7, :D] = Xs[rng.randint(0, N, size=len(Cs[::7])), :D] + 1e-3 * rng.normal(size=(len(Cs[::7]), D))   # near a training point
    alpha = rng.normal(size=N) * np.exp(rng.uniform(-3, 3, size=N))
    return Xs, Cs, alpha.astype(np.float64), 1.7, Dp


def write_input(path, Xs, Cs, alpha, constant, D):
    with open(path, "wb") as f:
        f.write(np.array([Xs.shape[0], Cs.shape[0], Xs.shape[1], D], dtype=np.int32).tobytes())
        f.write(np.float64(constant).tobytes())
        f.write(np.ascontiguousarray(Xs, dtype=np.float32).tobytes())
        f.write(np.ascontiguousarray(Cs, dtype=np.float32).tobytes())
        f.write(np.ascontiguousarray(alpha, dtype=np.float64).tobytes())


def run_driver(exe, splits, Xs, Cs, alpha, constant, D, tmp):
    """the driver's (9, M) output: run 1's and run 2's four arrays, then the exact mean"""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    write_input(fin, Xs, Cs, alpha, constant, D)
    res = subprocess.run([exe, str(splits), fin, fout], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return np.fromfile(fout, dtype=np.float64).reshape(9, -1)


def main():
    exe = sys.argv[1]
    outdir = sys.argv[2] if len(sys.argv) > 2 else HERE
    with tempfile.TemporaryDirectory() as tmp:
        for i, (N, M, D) in enumerate(CASES):
            Xs, Cs, alpha, constant, Dp = make_inputs(N, M, D, 100 + i)
            out = {}
            for s in SPLITS:
                o = run_driver(exe, s, Xs, Cs, alpha, constant, D, tmp)
                assert o[:4].tobytes() == o[4:8].tobytes(), "two runs of one build differ"
                assert np.isfinite(o[:4]).all()
                out["out_s%d" % s] = o[:4].copy()
            path = os.path.join(outdir, "screen_h2_bytes_n%d_m%d_d%d.npz" % (N, M, D))
            np.savez_compressed(path, Xs=Xs, Cs=Cs, alpha=alpha, constant=np.float64(constant), D=np.int32(D), **out)
            print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
