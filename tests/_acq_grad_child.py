"""Child process of tests/test_gpu_acq_grad_edges.py's alternate-path cases: the TGP_* tuning switches are read once per
process, so each selection of kernels gets its own process.  argv[1:]: cases "MODEL:m" -- the model of
tests/acq_grad_edge_cases.py fitted on a fresh handle and every quantity queried at the leading m rows of its base batch.
Prints one line "acq-grad-child " + JSON {case: judge() result}; the parent asserts the bars."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import turbo_amd as ta                      # noqa: E402
import acq_grad_edge_cases as ac            # noqa: E402
import cov_edge_cases as ec                 # noqa: E402

out = {}
for case in sys.argv[1:]:
    name, m = case.split(":")
    gp = ec.fit_handle(ta.NativeGP(0, ac.MODELS[name]["dtype"]), name)
    out[case] = ac.judge(name, "base", ac.query_all(gp, name, ac.points(name)[:int(m)]))
print("acq-grad-child " + json.dumps(out))
