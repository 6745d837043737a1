"""Child process of tests/test_gpu_lml_grad_edges.py's alternate-path cases: the TGP_* tuning switches are read once per
process, so each selection of kernels gets its own process.  argv[1:]: cases of tests/lml_grad_edge_cases.py, each run
through fit_grad on a fresh handle of the model's dtype.  Prints one line "lml-grad-child " + JSON
{case: [lml, grad...] as float.hex()}: the bits, for the parent to judge and to compare."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import turbo_amd as ta                      # noqa: E402
import lml_grad_edge_cases as lc            # noqa: E402

out = {}
for case in sys.argv[1:]:
    lml, grad = lc.fit_grad(ta.NativeGP(0, lc.config(case)["dtype"]), case)
    out[case] = [float(v).hex() for v in [lml] + list(grad)]
print("lml-grad-child " + json.dumps(out))
