"""NumPy restatement of the pruned sweep's speculative round (csrc/sweep_pruned.hpp: prune_pick4_kernel, prune_extras_kernel,
the leftover count of prune_scatter_kernel and sweep_pruned's hit / miss branch; DESIGN.md §4, TGP_PRUNE_SPEC).

The lb set's exact round also contracts the `extras`: of the second to fourth bound of each group (the runner-ups) the
`cap` largest, largest first.  The bar lb is the best exact value of the PICKS alone, the survivors are those of
prune_reference.survivors; when every survivor is an extra (a hit) the arg-max over picks + extras ends the sweep, otherwise
(a miss) the survivors are contracted as if the extras had never been."""
import math

import numpy as np

import prune_reference as pr

CAP = 128          # TGP_PRUNE_SPEC_CAP
NOT_TRIED, HIT, MISS = 0, 1, 2


def _order(ub, idx):
    """idx sorted by (bound descending, index ascending): the kernels' `better`"""
    idx = np.asarray(idx, dtype=np.int64)
    return idx[np.lexsort((idx, -np.asarray(ub, dtype=np.float64)[idx]))]


def picks_and_runner_ups(ub, top=pr.TOP):
    """prune_pick4_kernel: per group of ceil(M / top) consecutive candidates the four largest bounds (lowest index on ties);
    the first is the pick, the next three the runner-ups, -1 (IDX_NONE) where the group has no more members"""
    M = len(ub)
    gs = -(-M // top)
    picks, runner = [], []
    for g in range(0, M, gs):
        o = _order(ub, np.arange(g, min(g + gs, M)))
        picks.append(int(o[0]))
        runner.append([int(o[k]) if k < len(o) else -1 for k in (1, 2, 3)])
    return np.array(picks, dtype=np.int64), np.array(runner, dtype=np.int64).reshape(-1, 3)


def extras(ub, runner, cap=CAP):
    """prune_extras_kernel: the first `cap` runner-ups by (bound descending, index ascending), in that order"""
    real = runner[runner >= 0]
    return _order(ub, real)[:max(cap, 0)]


def leftover(surv, ex):
    """the survivors that are not among the extras (the scatter looks among its group's runner-ups)"""
    return int(np.sum(~np.isin(surv, ex)))


def _argmax(exact, idx):
    """(value, lowest index) as finalize + arg-max report it: a NaN never wins, its index still takes part"""
    idx = np.sort(np.asarray(idx, dtype=np.int64))
    vals = np.where(np.isnan(exact[idx]), -np.inf, exact[idx])
    j = int(np.argmax(vals))
    return float(vals[j]), int(idx[j])


def spec_argmax(exact, ub, top=pr.TOP, margin=pr.MARGIN, cap=CAP, direct=None):
    """the speculating schedule on host arrays: dict(value, index, lb, survivors, outcome, contracted) -- `contracted` the
    candidates whose exact value was formed before the final arg-max"""
    exact = np.asarray(exact, dtype=np.float64)
    ub = np.asarray(ub, dtype=np.float64)
    picks, runner = picks_and_runner_ups(ub, top)
    ex = extras(ub, runner, cap)
    if len(ex) == 0:                                            # nothing to speculate with: today's schedule
        v, i, n = pr.pruned_argmax(exact, ub, top, margin)
        surv = pr.survivors(ub, picks, _lb(exact, picks), margin)
        return dict(value=v, index=i, lb=_lb(exact, picks), survivors=n, outcome=NOT_TRIED,
                    contracted=np.sort(np.concatenate([picks, surv])))
    lb = _lb(exact, picks)                                      # the picks' blocks alone
    surv = pr.survivors(ub, picks, lb, margin)
    hit = leftover(surv, ex) == 0 and len(surv) <= len(ex) and (direct is None or len(surv) <= direct)
    # a miss contracts the survivors as if the extras had never been: nothing of the extras reaches the arg-max
    pool = np.concatenate([picks, ex]) if hit else np.concatenate([picks, surv])
    v, i = _argmax(exact, pool)
    return dict(value=v, index=i, lb=lb, survivors=len(surv), outcome=HIT if hit else MISS, contracted=np.sort(pool))


def _lb(exact, picks):
    ok = ~np.isnan(exact[picks])
    return float(exact[picks][ok].max()) if ok.any() else -math.inf


def covered(ub, lb, contracted, margin=pr.MARGIN):
    """the coverage predicate: every candidate whose bound reaches the bar was contracted"""
    need = np.nonzero(np.asarray(ub) >= pr.bar(lb, margin))[0]
    return bool(np.all(np.isin(need, contracted)))
