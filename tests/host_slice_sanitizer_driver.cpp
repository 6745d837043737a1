// Driver of tests/test_hyper_sample_sanitizers.py: the slice sampler of csrc/host_slice.hpp over the host backend
// (csrc/host_backend.cpp), compiled with -fsanitize=address,undefined.  A stand-alone program: CPU build only, never run on
// a GPU machine.  It walks every branch of the sampler: all coordinates free, fixed entries (lo == hi, the noise at -inf),
// intervals clipped at both bounds, non-PD proposals (rejected and counted), a non-PD start (handed back), thin > 1.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/turbogp.h"
#include "host_backend.hpp"
#include "host_slice.hpp"

struct Problem {
    int N, D;
    std::vector<double> X, y;
};

static int sample(tgp_host::HostGP &g, const Problem &p, int kernel, int n_ls, const std::vector<double> &t0,
                  const std::vector<double> &lo, const std::vector<double> &hi, const double *width, double jitter, int S, int burn,
                  int thin, uint64_t seed, std::vector<double> &theta, std::vector<double> &lml, int64_t &ev, int64_t &npd) {
    const int P = 2 + n_ls;
    theta.assign((size_t)S * P, NAN);
    lml.assign((size_t)S, NAN);
    std::vector<double> ls((size_t)n_ls);
    auto eval = [&](const double *th, double *f) {
        double c, noise;
        tgp::slice_unpack(th, n_ls, c, ls.data(), noise);
        return g.fit(p.X.data(), p.N, p.D, p.y.data(), kernel, c, ls.data(), n_ls, noise, jitter, 1, f, nullptr, nullptr);
    };
    if (tgp::slice_check_args(p.X.data(), p.N, p.D, p.y.data(), kernel, t0.data(), n_ls, lo.data(), hi.data(), jitter, S, burn, thin,
                              width, theta.data(), lml.data()))
        return TGP_BAD_ARG;
    return tgp::slice_sample(eval, P, t0.data(), lo.data(), hi.data(), width, S, burn, thin, seed, theta.data(), lml.data(), &ev, &npd);
}

int main() {
    unsigned s = 5u;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; };
    Problem p{10, 2, {}, {}};
    p.X.resize(20); p.y.resize(10);
    for (auto &v : p.X) v = rnd();
    for (int i = 0; i < 10; ++i) p.y[i] = std::sin(3 * p.X[2 * i]) + p.X[2 * i + 1];
    tgp_host::HostGP g;
    std::vector<double> theta, lml;
    int64_t ev = 0, npd = 0;
    // 1. everything free, ARD, thin 2
    {
        std::vector<double> t0 = {0.0, std::log(0.5), std::log(0.5), std::log(1e-2)};
        std::vector<double> lo = {std::log(1e-2), std::log(1e-2), std::log(1e-2), std::log(1e-5)}, hi = {std::log(1e2), std::log(10.0), std::log(10.0), 0.0};
        const int rc = sample(g, p, TGP_MATERN52, 2, t0, lo, hi, nullptr, 1e-10, 5, 2, 2, 7, theta, lml, ev, npd);
        if (rc != TGP_OK || ev < 5) { printf("free rc=%d ev=%lld\n", rc, (long long)ev); return 1; }
        for (size_t i = 0; i < theta.size(); ++i)
            if (!(theta[i] >= lo[i % 4] && theta[i] <= hi[i % 4])) { printf("outside the box\n"); return 1; }
        printf("free: ev=%lld not_pd=%lld lml=%.6f\n", (long long)ev, (long long)npd, lml[4]);
    }
    // 2. fixed constant, no noise term, a narrow box that clips both ends, wide steps
    {
        std::vector<double> t0 = {0.3, std::log(0.3), -INFINITY};
        std::vector<double> lo = {0.3, std::log(0.25), -INFINITY}, hi = {0.3, std::log(0.35), -INFINITY};
        const double width[3] = {1.0, 5.0, 1.0};
        const int rc = sample(g, p, TGP_RBF, 1, t0, lo, hi, width, 1e-8, 4, 0, 1, 8, theta, lml, ev, npd);
        if (rc != TGP_OK || theta[0] != 0.3 || !std::isinf(theta[2])) { printf("fixed rc=%d\n", rc); return 1; }
        printf("fixed: ev=%lld lml=%.6f\n", (long long)ev, lml[3]);
    }
    // 3. duplicated rows 1e-9 apart, no jitter, no noise: long length scales are not PD -> rejected and counted
    {
        Problem q{8, 1, {}, {}};
        for (int i = 0; i < 4; ++i) { const double v = rnd(); q.X.push_back(v); q.y.push_back(std::sin(4 * v)); }
        for (int i = 0; i < 4; ++i) { q.X.push_back(q.X[(size_t)i] + 1e-9); q.y.push_back(q.y[(size_t)i]); }
        std::vector<double> t0 = {0.0, std::log(1e-8), -INFINITY};
        std::vector<double> lo = {0.0, std::log(1e-9), -INFINITY}, hi = {0.0, std::log(10.0), -INFINITY};
        const double width[3] = {1.0, 6.0, 1.0};
        int rc = sample(g, q, TGP_RBF, 1, t0, lo, hi, width, 0.0, 4, 1, 1, 9, theta, lml, ev, npd);
        if (rc != TGP_OK || npd < 1) { printf("not-pd proposals rc=%d npd=%lld\n", rc, (long long)npd); return 1; }
        printf("not-pd: ev=%lld not_pd=%lld\n", (long long)ev, (long long)npd);
        t0[1] = 0.0;                                                    // ... and a start that is not PD is handed back
        rc = sample(g, q, TGP_RBF, 1, t0, lo, hi, width, 0.0, 2, 0, 1, 9, theta, lml, ev, npd);
        if (rc != TGP_NOT_PD || ev != 1) { printf("not-pd start rc=%d\n", rc); return 1; }
    }
    // 4. the argument rules
    {
        std::vector<double> t0 = {0.0, 0.0, 0.0}, lo = {-1, -1, -1}, hi = {1, 1, 1}, bad = {0.0, 2.0, 0.0};
        if (sample(g, p, TGP_RBF, 1, t0, lo, hi, nullptr, 0.0, 0, 0, 1, 1, theta, lml, ev, npd) != TGP_BAD_ARG ||
            sample(g, p, TGP_RBF, 1, t0, lo, hi, nullptr, 0.0, 65, 0, 1, 1, theta, lml, ev, npd) != TGP_BAD_ARG ||
            sample(g, p, TGP_RBF, 1, t0, lo, hi, nullptr, 0.0, 2, 0, 0, 1, theta, lml, ev, npd) != TGP_BAD_ARG ||
            sample(g, p, TGP_RBF, 1, t0, hi, lo, nullptr, 0.0, 2, 0, 1, 1, theta, lml, ev, npd) != TGP_BAD_ARG ||
            sample(g, p, TGP_RBF, 1, bad, lo, hi, nullptr, 0.0, 2, 0, 1, 1, theta, lml, ev, npd) != TGP_BAD_ARG) {
            printf("a bad argument was accepted\n");
            return 1;
        }
    }
    printf("ok\n");
    return 0;
}
