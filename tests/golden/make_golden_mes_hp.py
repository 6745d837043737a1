#!/usr/bin/env python3
"""tests/golden/mes_hp_grid.json: h(gamma) and dh/dgamma of max-value entropy search on the grid of
tests/mes_edge_cases.py from mpmath, as decimal strings of 40 digits -- what tests/test_mes_reference_hp.py holds the
80-bit reference to where mpmath is not installed.  Needs mpmath; data only.

    h = gamma r / 2 - log Phi,   dh = -(r / 2)(1 + gamma^2 + gamma r),   r = phi / Phi

formed with enough digits for the cancellation (gamma^4 in dh): 50 beyond what -log10 of the cancelling terms' ratio takes.
gamma > 0: log Phi = log1p(-Q), Q = erfc(gamma / sqrt 2) / 2 (1 - Q at fixed digits loses Q beyond gamma = 16).
gamma < -150.5: Phi = phi m with Mills' ratio m from its asymptotic series in 1 / gamma^2, 60 terms (the 60th is below
1e-150 of the sum there) -- mpmath's erfc does not take 1e300."""
import json
import os
import sys

import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(1, os.path.dirname(os.path.dirname(HERE)))
import mes_edge_cases as me  # noqa: E402

DIGITS = 40


def h_dh(gamma):
    """(h, dh) of the f64 gamma as mpf, at a precision set for that gamma"""
    x = abs(float(gamma))
    mp.mp.dps = 50 + DIGITS + (int(4 * mp.log10(x)) + 1 if x > 1 else 0)
    g = mp.mpf(float(gamma))
    if g < -150.5:
        x = -g
        t = 1 / (x * x)
        m, term = mp.mpf(0), mp.mpf(1)
        for k in range(60):
            m += term
            term *= -(2 * k + 1) * t
        m /= x
        r = 1 / m
        return -x * r / 2 + x * x / 2 + mp.log(mp.sqrt(2 * mp.pi)) - mp.log(m), -r / 2 * (1 + g * g + g * r)
    if g > 1e5:                                   # exp(-gamma^2 / 2) is below 1e-2e9: 0 in every format here
        return mp.mpf(0), mp.mpf(0)
    if g <= 0:
        P = mp.erfc(-g / mp.sqrt(2)) / 2
        lp = mp.log(P)
    else:
        Q = mp.erfc(g / mp.sqrt(2)) / 2
        P = 1 - Q
        lp = mp.log1p(-Q)
    r = mp.npdf(g) / P
    return g * r / 2 - lp, -r / 2 * (1 + g * g + g * r)


def main():
    g = me.grid()
    rows = []
    for x in g:
        h, dh = h_dh(x)
        rows.append([float(x).hex(), mp.nstr(h, DIGITS, min_fixed=0, max_fixed=0), mp.nstr(dh, DIGITS, min_fixed=0, max_fixed=0)])
    with open(os.path.join(HERE, "mes_hp_grid.json"), "w") as f:
        json.dump(dict(columns=["gamma (f64, hex)", "h", "dh/dgamma"], digits=DIGITS, rows=rows), f, indent=0)
    print("wrote %d rows" % len(rows))


if __name__ == "__main__":
    main()
