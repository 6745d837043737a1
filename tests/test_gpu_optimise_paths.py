"""What the optimiser entries (tgp_fit_optimise, tgp_fit_lbfgsb, tgp_acq_refine, tgp_acq_lbfgsb, tgp_hyper_sample) return
on every path their host code takes -- one launch and streams, small and general refine, the lock-step L-BFGS-B, fixed
entries, no noise term, a matrix that is not positive definite, the iteration limits around the general refine's poll --
and what they refuse, with the exact texts.

The bytes are held to tests/golden/optimise_paths_parent.json: recorded from the build BEFORE these entries moved into
csrc/api_optimise.hpp over host_lbfgsb.hpp's one walk (_optimise_paths_child.py --record), a SHA-256 of every returned
array with the evaluation count, the statuses, the return code and tgp_last_error's text per case.  The refactor changed
no arithmetic, so every case has to come back bit for bit.

The cases live in _optimise_paths_child.py.  csrc/tuning.hpp reads the TGP_* switches once per process, so the default
selection runs here and every other one in a child process of its own."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _optimise_paths_child as cases      # noqa: E402

with open(cases.FIXTURE) as _f:
    PARENT = json.load(_f)
_results = {}


def _here(group):
    if group not in _results:
        _results[group] = json.loads(json.dumps(cases.GROUPS[group]()))     # (as the fixture went through JSON)
    return _results[group]


def _child(groups, **env):
    """the groups' results from a child process under `env` (one process per selection of switches, shared by the tests)"""
    key = (tuple(groups), tuple(sorted(env.items())))
    if key not in _results:
        e = dict(os.environ)
        e.update(env)
        out = subprocess.run([sys.executable, os.path.join(HERE, "_optimise_paths_child.py"), *groups], env=e, capture_output=True,
                             text=True, timeout=300)
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("optimise-paths ")]
        assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-4000:]
        _results[key] = json.loads(lines[-1][len("optimise-paths "):])
    return _results[key]


def _same(got, want):
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


@pytest.mark.parametrize("group", cases.RECORDED)
def test_returns_the_parents_bytes(group):
    _same(_here(group), PARENT[group])


@pytest.mark.parametrize("group", cases.RECORDED)
def test_returns_the_parents_bytes_event_timed(group):
    """TGP_POLL_US=0: every short call completes by events and hipStreamSynchronize instead of its doorbell.  The fixture's
    bytes again -- but for ten N = 30 cases of tgp_acq_lbfgsb, whose every round is a tgp_acq_grad: event-timed, that entry
    runs its unfused kernel sequence and differs in the last bits (in the parent's build too), so the parent's event-timed
    bytes of those cases are recorded beside the others ("refine_event_timed": same counts and statuses)"""
    want = dict(PARENT[group], **PARENT["refine_event_timed"]) if group == "refine" else PARENT[group]
    _same(_child(cases.RECORDED, TGP_POLL_US="0")[group], want)


def test_the_cases_reach_their_branches():
    """what the fixture's cases are there for, said of the results themselves"""
    L = cases._L()
    h, r = _here("hyper"), _here("refine")
    print(json.dumps(h, indent=1), json.dumps(r, indent=1))
    assert all(v["rc"] == L.OK for v in h.values()) and all(v["rc"] == L.OK for v in r.values())
    for entry in ("optimise", "lbfgsb"):
        assert h["N129 all fixed / " + entry]["ev"] == 3 and h["N129 all fixed / " + entry]["status"] == [1, 1, 1]
        assert h["N30 all fixed / lbfgsb"]["ev"] == 3
        # not positive definite wherever the box lets a start go: a status per start, not a failure of the call
        assert h["not PD streams / " + entry]["rc"] == L.OK and h["not PD streams / " + entry]["status"] == [1, 1, 1]
        assert h["not PD one launch / " + entry]["rc"] == L.OK
        # max_iter bounds accepted iterations: one iteration is at least two evaluations per start
        assert h["N129 max_iter 1 / " + entry]["ev"] >= 6 and h["N129 max_iter 2 / " + entry]["ev"] > h["N129 max_iter 1 / " + entry]["ev"]
    # the general refine counts iterations (polled at every fourth and at the limit), the small one the slowest restart's evaluations
    for it in (1, 3, 4, 5):
        assert r["N200 refine EI R3 it%d" % it]["rc"] == L.OK and 1 <= r["N200 refine EI R3 it%d" % it]["ev"] <= it + 1
        assert r["N30 refine EI R3 it%d" % it]["rc"] == L.OK and r["N30 lbfgsb MES R3 it%d" % it]["rc"] == L.OK
    assert r["N200 lbfgsb UCB R3 it40"]["ev"] > r["N200 lbfgsb UCB R1 it5"]["ev"]          # the sum over restarts


REFUSED = {
    " R=0": "need X0, lo, hi, x_out, val_out and 1 <= R <= 4096", " R=4097": "need X0, lo, hi, x_out, val_out and 1 <= R <= 4096",
    " max_iter=0": "max_iter >= 1", " lo > hi": "need lo <= hi in every dimension", " NaN bound": "need lo <= hi in every dimension",
    " sf": "sf must be +1 or -1", " R=0, max_iter=0, lo > hi": "need X0, lo, hi, x_out, val_out and 1 <= R <= 4096",
    " max_iter=0, lo > hi": "max_iter >= 1",
}
HYPER_REFUSED = {
    " S=65": "needs N >= 1, 1 <= D <= 4096, n_ls 1 or D, 1 <= S <= 64, max_iter >= 1",
    " S=0": "needs N >= 1, 1 <= D <= 4096, n_ls 1 or D, 1 <= S <= 64, max_iter >= 1",
    " max_iter=0": "needs N >= 1, 1 <= D <= 4096, n_ls 1 or D, 1 <= S <= 64, max_iter >= 1",
    " n_ls=3": "needs N >= 1, 1 <= D <= 4096, n_ls 1 or D, 1 <= S <= 64, max_iter >= 1",
    " bound inf": "bounds must be finite with lo <= hi (the noise entry may be fixed at -inf: no noise term)",
    " bound nan": "bounds must be finite with lo <= hi (the noise entry may be fixed at -inf: no noise term)",
    " bound noise hi = -inf alone": "bounds must be finite with lo <= hi (the noise entry may be fixed at -inf: no noise term)",
    " lo > hi": "bounds must be finite with lo <= hi (the noise entry may be fixed at -inf: no noise term)",
    " NULL": "need X, y, theta0, log_lo, log_hi, theta_out, f_out",
}
HOST_TEXT = ("%s: not available on the host backend (a TGP_DEVICE_HOST handle keeps a reloaded model queryable: fit, predict, "
             "acquisition; the rest needs the GPU)")


def test_refusals_and_their_texts():
    L = cases._L()
    res = _here("refusals")
    for entry in ("refine", "lbfgsb"):
        fn = "tgp_acq_" + entry
        for case, text in REFUSED.items():
            assert (res[entry + case]["rc"], res[entry + case]["err"]) == (L.BAD_ARG, fn + ": " + text), (entry, case)
            assert res[entry + case]["ev"] == -7                                   # nothing was written
        assert (res[entry + " not fitted"]["rc"], res[entry + " not fitted"]["err"]) == (L.NOT_FITTED, fn + ": no fitted model")
        assert (res["host acq_" + entry]["rc"], res["host acq_" + entry]["err"]) == (L.BAD_ARG, HOST_TEXT % fn)
    assert (res["refine MES"]["rc"], res["refine MES"]["err"]) == (L.BAD_ARG, "tgp_acq_refine: unknown acquisition")
    assert (res["lbfgsb acq 6"]["rc"], res["lbfgsb acq 6"]["err"]) == (L.BAD_ARG, "tgp_acq_lbfgsb: unknown acquisition")
    for entry in ("optimise", "lbfgsb"):
        fn = "tgp_fit_" + entry
        for case, text in HYPER_REFUSED.items():
            assert (res[fn[4:] + case]["rc"], res[fn[4:] + case]["err"]) == (L.BAD_ARG, fn + ": " + text), (entry, case)
        assert (res["host " + fn[4:]]["rc"], res["host " + fn[4:]]["err"]) == (L.BAD_ARG, HOST_TEXT % fn)
    assert res["hyper_sample S=65"] == dict(rc=L.BAD_ARG, err="tgp_hyper_sample: needs 1 <= S <= 64, burn >= 0, thin >= 1")
    assert res["hyper_sample n_ls=3"] == dict(rc=L.BAD_ARG, err="tgp_hyper_sample: needs N >= 1, 1 <= D <= 4096, n_ls 1 or D")
    assert res["hyper_sample bound inf"] == dict(
        rc=L.BAD_ARG, err="tgp_hyper_sample: bounds must be finite with lo <= hi (the noise entry may be fixed at -inf: no noise term)")
    assert res["host hyper_sample"] == dict(rc=L.OK, ran=True, finite=True)      # (the one entry the host backend has)
    s = _here("hyper_sample")["not PD at theta0"]
    assert s["rc"] == L.NOT_PD and s["err"].startswith("tgp_hyper_sample: at theta0: ") and s["ev"] == 1 and s["not_pd"] == 0


def test_the_thread_count_does_not_show():
    """TGP_HYPER_THREADS=1 (every start on the caller's handle, one after the other) against the default (a worker handle
    and a thread per start, five starts on four threads): the same bytes, counts and statuses.  (Not tgp_last_error's
    text behind a call that succeeded: a start's "not positive definite" was said on the handle that evaluated it.)"""
    def quiet(res):
        return {k: {f: v[f] for f in v if f != "err" or v["rc"] != 0} for k, v in res.items()}
    _same(quiet(_child(("hyper",), TGP_HYPER_THREADS="1")["hyper"]), quiet(_here("hyper")))


def test_fit_optimise_is_fit_lbfgsb_off_the_one_launch_path():
    """N > 128, Dp > 64, no noise term, or TGP_SMALL=0: tgp_fit_optimise IS tgp_fit_lbfgsb"""
    h = _here("hyper")
    streams = [k[:-len(" / lbfgsb")] for k in h if k.endswith(" / lbfgsb") and (k.startswith("N129") or "D65" in k or "no noise" in k)]
    assert len(streams) == 11
    for name in streams:
        assert h[name + " / optimise"] == h[name + " / lbfgsb"], name
    assert h["N30 / optimise"] != h["N30 / lbfgsb"]                       # (one launch: a projected L-BFGS of its own)
    off = _child(("hyper_n30",), TGP_SMALL="0")["hyper_n30"]
    assert off["N30 / optimise"] == off["N30 / lbfgsb"]
