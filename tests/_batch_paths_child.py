"""Child process of test_read_once_switches_in_a_child_process: TGP_SMALL, TGP_MID, TGP_TILE, TGP_SLAB_GB and TGP_KS_JS
are read once per process, so each setting gets its own process.  At one size per first-sweep path (N = 100 small,
200 mid, 600 general) tgp_sweep_batch is held to the reference under teacher forcing (f64 limits) and q = 1 to tgp_sweep
bit for bit; prints 'batch-paths ok'."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import batch_reference as br                                                      # noqa: E402
from oracle import gp_oracle as o                                                 # noqa: E402
from test_gpu_batch_coverage import _assert_q1_is_the_sweep, _check_parity, _gp, _problem   # noqa: E402

for N, kind, M in ((100, "matern52", 3000), (200, "rbf", 3000), (600, "matern32", 7000)):
    X, y, ls, Xc, Xp = _problem(N, 17, M, 500 + N, ard=True, n_pending=3)
    gp = _gp("f64", X, y, kind, 1.3, ls, 1e-3, 1e-10, True, Xc)
    om = o.fit(X, y, kind, 1.3, ls, 1e-3, 1e-10, True)
    _check_parity(gp, om, Xc, 8, br.KB, 0.0, Xp, "ei", -1.0, float(y.min()), 0.01)
    _check_parity(gp, om, Xc, 6, br.CL, float(y.max()), None, "pi", 1.0, float(y.max()), 0.0)
    _assert_q1_is_the_sweep(gp, y)
    gp.close()
print("batch-paths ok")
