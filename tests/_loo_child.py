"""Child process of tests/test_gpu_loo.py: the TGP_* tuning switches are read once per process, so a setting gets its own
process.  argv[1]: "lml" (fit_grad: under TGP_SMALL=0 that is the blocked route tgp_fit_loo_grad always takes) or "loo"
(fit_loo_grad); argv[2:]: cases of tests/loo_edge_cases.py, each on a fresh handle of the model's dtype.  Prints one line
"loo-child " + JSON {case: [lml] or [lml, loo, grad...] as float.hex()}: the bits, for the parent to judge and to compare."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import turbo_amd as ta                      # noqa: E402
import loo_edge_cases as le                 # noqa: E402

out = {}
for case in sys.argv[2:]:
    gp = ta.NativeGP(0, le.config(case)["dtype"])
    if sys.argv[1] == "lml":
        vals = [le.lc.fit_grad(gp, case)[0]]
    else:
        r = le.fit_loo_grad(gp, case)
        vals = [r["lml"], r["loo"]] + list(r["grad"])
    out[case] = [float(v).hex() for v in vals]
print("loo-child " + json.dumps(out))
