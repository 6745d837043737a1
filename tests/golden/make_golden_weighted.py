"""Writes tests/golden/weighted_eref.json and tests/golden/weighted_grad_eref.json: the NumPy reference's OWN errors, which
the GPU tests' bars are made of (tests/weighted_reference.py, tests/weighted_cases.py).  Run from the repository root:
    python tests/golden/make_golden_weighted.py
  weighted_eref.json       e_ref: the worst relative error of the f64 log Phi (scipy.special.log_ndtr) against mpmath on the
                           set Z_SET (relative to max(|log Phi|, the smallest normal double): log Phi(40) = -3.7e-350 rounds to -0.0), and the
                           per-z figures
  weighted_grad_eref.json  per gradient case, the f64 restatement's worst error against the 80-bit closed form: of the
                           value (relative) and of the gradient (entry by entry, over that entry's sum of absolute terms)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mpmath as mp  # noqa: E402
import numpy as np  # noqa: E402

import weighted_cases as wc  # noqa: E402
import weighted_reference as wr  # noqa: E402


def log_phi_errors():
    per = {}
    with mp.workdps(60):
        for z in wr.Z_SET:
            ref = wr.logphi_mp(z)
            got = mp.mpf(float(wr.logphi(np.array([z]))[0][0]))
            per[repr(z)] = float(abs(got - ref) / max(abs(ref), mp.mpf(wr.TINY)))
    return per


if __name__ == "__main__":
    per = log_phi_errors()
    with open(os.path.join(HERE, "weighted_eref.json"), "w") as f:
        json.dump(dict(e_ref=max(per.values()), per_z=per), f, indent=1, sort_keys=True)
    cases = {}
    for name in wc.GRAD_CASES:
        v, g, _ = wc.grad_references(name, f64=True)
        ev, eg = wc.grad_errors(name, v, g)
        cases[name] = dict(value=ev, grad=eg)
        print(name, cases[name])
    with open(os.path.join(HERE, "weighted_grad_eref.json"), "w") as f:
        json.dump(dict(cases=cases), f, indent=1, sort_keys=True)
