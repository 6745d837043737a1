"""Writes tests/golden/ehvi_eref.json: the NumPy reference's OWN error, which the GPU tests' bars are made of
(tests/ehvi_reference.py).  Run from the repository root:
    python tests/golden/make_golden_ehvi.py
  e_ref  the worst error of the f64 H(z) = phi(z) + z Phi(z) of tests/ehvi_reference.py against mpmath over Z_SET (from -38
         through 0 to +40), relative to (2 + min(z, 0)^2) H(z): that weight is H's condition number in z (|z Phi(z) / H(z)|
         <= 2 + z^2 for z < 0, <= 1 otherwise), and z itself carries about 2 u.  H(-38) = 7e-318 is below the smallest
         normal double and has no full-precision f64 representation: there the error is taken relative to that smallest normal
  per_z  the figure of every z
  grad   per gradient case of tests/ehvi_cases.py, the f64 NumPy restatement's worst error against the 80-bit closed form,
         entry by entry over that entry's sum of absolute terms: what f64 arithmetic makes of the case's conditioning (the
         coefficients are steep functions of posteriors that themselves carry N u of their own terms), as
         tests/golden/weighted_grad_eref.json holds it for the weighted gradient
The reference is measured, not the library."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mpmath as mp  # noqa: E402
import numpy as np  # noqa: E402

import ehvi_cases as ec  # noqa: E402
import ehvi_reference as er  # noqa: E402


def h_errors():
    per = {}
    with mp.workdps(80):
        for z in er.Z_SET:
            ref = er.H_mp(z)
            got = mp.mpf(float(er.H(np.array([z]))[0]))
            per[repr(z)] = float(abs(got - ref) / ((2 + min(z, 0.0) ** 2) * max(ref, mp.mpf(er.TINY))))
    return per


if __name__ == "__main__":
    per = h_errors()
    for z in er.Z_SET:
        print(z, per[repr(z)])
    grad = {}
    for name in ec.GRAD_CASES:
        grad[name] = ec.grad_error(name, ec.grad_references(name, f64=True)[1])
        print(name, grad[name])
    with open(os.path.join(HERE, "ehvi_eref.json"), "w") as f:
        json.dump(dict(e_ref=max(per.values()), per_z=per, grad=grad), f, indent=1, sort_keys=True)
