// Driver of tests/test_host_lbfgs.py::test_lbfgsb_under_sanitizers: csrc/host_lbfgsb.hpp compiled with
// -fsanitize=address,undefined and walked over objectives that reach every branch -- memory wrap-around (more than 10
// pairs), active bounds at the Cauchy point, the subspace step's projection and back-tracking, a wall of +inf, a start
// inside the wall, lo == hi, no bounds at all, the iteration limit (GPU sanitizers are not available on this pool: CPU
// build only).  Then three of the walks again in lock-step -- a plain one, one whose first trial hits the wall (it ends on
// a step from the cache), one stopped by max_iter = 1 -- which must print what each prints alone.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "host_lbfgsb.hpp"

static double rosen(const std::vector<double> &x, std::vector<double> &g, double wall) {
    const size_t P = x.size();
    if (x[0] > wall) { for (auto &v : g) v = 0.0; return INFINITY; }
    double f = 0.0;
    for (auto &v : g) v = 0.0;
    for (size_t i = 0; i + 1 < P; ++i) {
        const double a = x[i + 1] - x[i] * x[i], b = 1.0 - x[i];
        f += 100.0 * a * a + b * b;
        g[i] += -400.0 * a * x[i] - 2.0 * b;
        g[i + 1] += 200.0 * a;
    }
    return f;
}

struct Case { int P; double lo, hi, x0, wall; int max_iter; };

struct Run {
    Case c;
    std::vector<double> lo, hi, gt;
    tgp::LbfgsbWalk walk;
    static std::vector<double> bound(const Case &c, double v, int open, double inf) {
        std::vector<double> b((size_t)c.P, v);
        if (c.P == 20) b[(size_t)open] = inf;                              // half-open coordinates among boxed ones
        return b;
    }
    explicit Run(const Case &c_)
        : c(c_), lo(bound(c_, c_.lo, 7, -INFINITY)), hi(bound(c_, c_.hi, 3, INFINITY)), gt((size_t)c_.P),
          walk(std::vector<double>((size_t)c_.P, c_.x0).data(), lo.data(), hi.data(), c_.P, c_.max_iter, 1e-5, 2.220446049250313e-09) {}
    bool advance() {                                                       // one evaluation, if the walk wants one
        if (!walk.wants_eval()) return false;
        const double f = rosen(walk.xt, gt, c.wall);
        walk.tell(f, gt);
        return true;
    }
    std::string line() const {
        const tgp::HostLbfgsb &opt = walk.opt;
        bool inside = true;
        for (int k = 0; k < c.P; ++k) inside = inside && opt.x[(size_t)k] >= lo[(size_t)k] && opt.x[(size_t)k] <= hi[(size_t)k];
        char buf[160];
        snprintf(buf, sizeof buf, "P=%d status=%d iters=%d evals=%d f=%.6g inside=%d", c.P, opt.status, opt.iters, (int)walk.evals,
                 opt.phi, (int)inside);
        return buf;
    }
};

int main() {
    const Case cases[] = {{2, -5, 5, -1.2, 1e9, 15000}, {66, -5, 5, -1.2, 1e9, 15000}, {20, -0.5, 0.8, 0.0, 1e9, 15000},
                          {5, -2, 2, -1.5, 0.3, 15000}, {3, -2, 2, 1.0, 0.5, 15000}, {8, -INFINITY, INFINITY, -1.2, 1e9, 15000},
                          {12, -5, 5, -1.2, 1e9, 7}, {4, 0.5, 0.5, 0.5, 1e9, 15000}};
    for (const Case &c : cases) {
        Run r(c);
        while (r.advance()) {}
        printf("%s\n", r.line().c_str());
    }
    // lock-step: the walks finish at different rounds
    const Case three[] = {{2, -5, 5, -1.2, 1e9, 15000}, {2, -2, 2, 0.0, 0.1, 15000}, {12, -5, 5, -1.2, 1e9, 1}};
    std::vector<Run> together(three, three + 3);
    for (bool any = true; any;) {
        any = false;
        for (Run &r : together) any = r.advance() || any;
    }
    int differ = 0;
    for (int i = 0; i < 3; ++i) {
        Run alone(three[i]);
        while (alone.advance()) {}
        printf("alone %s\nlockstep %s\n", alone.line().c_str(), together[(size_t)i].line().c_str());
        differ += alone.line() != together[(size_t)i].line();
    }
    return differ;
}
