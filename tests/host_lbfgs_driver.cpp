// Test driver (CPU): csrc/host_lbfgsb.hpp behind a C entry so the walk the library's optimiser entries run
// (LbfgsbWalk: tgp_fit_lbfgsb's starts, tgp_acq_lbfgsb's restarts in lock-step) can be exercised without a GPU, on
// objectives supplied by the test (ctypes callback).
//   g++ -O2 -std=c++17 -shared -fPIC -I turbo_amd/csrc tests/host_lbfgs_driver.cpp -o <tmp>/libhost_lbfgs_test.so
#include "host_lbfgsb.hpp"

// R walks in lock-step, as tgp_acq_lbfgsb drives them: every round asks each walk in turn and evaluates the points wanted.
// x (R, P) in and out; max_iter, f_out, evals_out, iters_out, status_out (R,)
extern "C" void host_lbfgs_lockstep(double (*fun)(const double *x, double *grad, void *ctx), void *ctx, int P, int R, double *x,
                                    const double *lo, const double *hi, const int *max_iter, double pgtol, double ftol,
                                    double *f_out, int *evals_out, int *iters_out, int *status_out) {
    std::vector<tgp::LbfgsbWalk> walks;
    walks.reserve((size_t)R);
    for (int r = 0; r < R; ++r) walks.emplace_back(x + r * P, lo, hi, P, max_iter[r], pgtol, ftol);
    std::vector<double> gt((size_t)P);
    for (bool any = true; any;) {
        any = false;
        for (tgp::LbfgsbWalk &w : walks) {
            if (!w.wants_eval()) continue;
            const double f = fun(w.xt.data(), gt.data(), ctx);
            w.tell(f, gt);
            any = true;
        }
    }
    for (int r = 0; r < R; ++r) {
        const tgp::LbfgsbWalk &w = walks[(size_t)r];
        for (int k = 0; k < P; ++k) x[r * P + k] = w.opt.x[(size_t)k];
        f_out[r] = w.opt.phi;
        evals_out[r] = (int)w.evals;
        iters_out[r] = w.opt.iters;
        status_out[r] = w.opt.status;
    }
}

extern "C" int host_lbfgs_minimise(double (*fun)(const double *x, double *grad, void *ctx), void *ctx, int P, double *x,
                                   const double *lo, const double *hi, int max_iter, double pgtol, double ftol,
                                   double *f_out, int *evals_out, int *iters_out) {
    int status = 0;
    host_lbfgs_lockstep(fun, ctx, P, 1, x, lo, hi, &max_iter, pgtol, ftol, f_out, evals_out, iters_out, &status);
    return status;
}
