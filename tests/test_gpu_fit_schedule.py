"""The blocked fit's schedule (csrc/fit_plan.hpp, csrc/fit_blocked.hpp) under every selection of its
switches: one child process per selection (tests/_fit_schedule_child.py -- csrc/tuning.hpp reads the table once per
process), which holds every fit against the oracle (LML rel 1e-9, L rtol 1e-8 / atol 1e-11, the f64 sweep 1e-7, the f32
sweep 5e-3) and prints the digests of L, Linv, alpha and the sweep.

The selections that only re-schedule the same arithmetic must leave the same BYTES as TGP_OB=256 alone:
* fused / unfused / mixed panels, TGP_GEMM64=reg, a zero-filled Linv, more of the sweep's front inside the fit, the
  handle on a private stream with the background stream on loan and without: L, Linv, alpha, the f64 sweep, the f32 sweep;
* the inverse level by level (TGP_BGINV=0) and its 64 -> 128 level in three launches: L;
* TGP_OB=1024 at Np = 1792 falls back to 512 (a tail of 768 is no power of two): everything TGP_OB=512 leaves;
* the f32 sweep started inside the fit (tgp_set_overlap(2)) is the serial one."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OB256 = dict(TGP_OB="256")
# id -> (switches, flags of the child)
SELECTIONS = {
    "default": ({}, ()),
    "ob256": (OB256, ("serial",)),
    "ob256-levels": (dict(OB256, TGP_BGINV="0"), ()),
    "ob256-unfused": (dict(OB256, TGP_PANEL_FUSE="0"), ()),
    "ob256-mixed": (dict(OB256, TGP_PANEL_FUSE_TILES="20"), ()),
    "ob256-la0": (dict(OB256, TGP_PANEL_LA="0"), ()),
    "ob256-panel3": (dict(OB256, TGP_PANEL="3"), ()),
    "ob256-panel0-generic": (dict(OB256, TGP_PANEL="0", TGP_INNER="gemm64"), ()),
    "ob256-glds": (dict(OB256, TGP_TRAIL64="0", TGP_MERGE64="0"), ()),
    "ob256-level64": (dict(OB256, TGP_LEVEL64_FUSED="0"), ()),
    "ob256-reg": (dict(OB256, TGP_GEMM64="reg"), ()),
    "ob256-zero": (dict(OB256, TGP_LINV_ZERO="1"), ()),
    "ob256-pretiles": (dict(OB256, TGP_PRE_TILES="2"), ()),
    "ob256-private": (OB256, ("private",)),
    "ob256-private-inline": (dict(OB256, TGP_BG_LEASE="0"), ("private",)),
    "ob1024-tail": (dict(TGP_OB="1024"), ("tail",)),
    "ob512": (dict(TGP_OB="512"), ("tail",)),
}
SAME_BYTES = ["ob256-unfused", "ob256-mixed", "ob256-reg", "ob256-zero", "ob256-pretiles", "ob256-private", "ob256-private-inline"]
SAME_L = ["ob256-levels", "ob256-level64"]
F64 = ["f64 N=1100", "f64 N=600", "f64 N=129"]
F32 = "f32 N=600 overlap=2"
_results = {}


def child(sel):
    """fit -> record of the selection's child process (run once, shared by the cases that compare against it)"""
    if sel not in _results:
        switches, flags = SELECTIONS[sel]
        env = {k: v for k, v in os.environ.items() if not k.startswith("TGP_") or k == "TGP_LIBRARY"}
        env.update(switches)
        out = subprocess.run([sys.executable, os.path.join(HERE, "_fit_schedule_child.py"), *flags], env=env, capture_output=True,
                             text=True, timeout=300)
        print("==", sel, " ".join("%s=%s" % kv for kv in sorted(switches.items())), *flags)
        print(out.stdout)
        assert out.returncode == 0 and out.stdout.rstrip().endswith("fit-schedule done"), out.stdout[-2000:] + out.stderr[-4000:]
        recs = [json.loads(ln[len("fit-schedule "):]) for ln in out.stdout.splitlines() if ln.startswith("fit-schedule {")]
        _results[sel] = {r["fit"]: r for r in recs}
    return _results[sel]


@pytest.mark.parametrize("sel", list(SELECTIONS))
def test_fit_schedule(sel):
    got = child(sel)
    tail = "tail" in SELECTIONS[sel][1]
    assert sorted(got) == sorted(F64 + [F32] + (["f64 N=1700"] if tail else []) + (["f32 N=600 overlap=0"] if sel == "ob256" else []))
    if sel in SAME_BYTES:
        ref = child("ob256")
        for fit in F64 + [F32]:
            assert got[fit] == ref[fit], (fit, got[fit], ref[fit])
    if sel in SAME_L:
        ref = child("ob256")
        for fit in F64:
            assert got[fit]["L"] == ref[fit]["L"], (fit, got[fit], ref[fit])
    if sel == "ob1024-tail":
        ref = child("ob512")["f64 N=1700"]
        assert got["f64 N=1700"] == ref, (got["f64 N=1700"], ref)
    if sel == "ob256":
        serial = dict(got["f32 N=600 overlap=0"], fit=F32)
        assert got[F32] == serial, (got[F32], serial)
