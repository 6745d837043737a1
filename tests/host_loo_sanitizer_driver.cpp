// Driver of tests/test_loo_reference.py::test_host_backend_loo_under_sanitizers: the host backend's leave-one-out
// cross-validation (turbo_amd/csrc/host_backend.cpp: HostGP::loo) at N = 1, 65 and 257, compiled with
// -fsanitize=address,undefined.  A stand-alone program: CPU build only, never run on a GPU machine.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/turbogp.h"
#include "host_backend.hpp"

int main() {
    const int D = 3;
    unsigned s = 91u;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; };
    tgp_host::HostGP g;
    if (g.loo(nullptr, nullptr, nullptr, nullptr) != TGP_NOT_FITTED) { printf("an unfitted model answered\n"); return 1; }
    for (int N : {1, 65, 257}) {
        std::vector<double> X(N * D), y(N), ls(D, 0.6);
        for (auto &v : X) v = rnd();
        for (int i = 0; i < N; ++i) y[i] = 1.5 + std::sin(3 * X[i * D]) + X[i * D + 1] + 0.02 * (rnd() - 0.5);
        int rc = g.fit(X.data(), N, D, y.data(), N == 65 ? TGP_MATERN12 : TGP_RBF, 1.3, ls.data(), N == 257 ? D : 1, 1e-3, 1e-10, 1,
                       nullptr, nullptr, nullptr);
        if (rc != TGP_OK) { printf("fit N=%d rc=%d %s\n", N, rc, g.err.c_str()); return 1; }
        std::vector<double> resid(N), sigma(N), lpd(N);
        double loo = 0.0, only = 0.0;
        rc = g.loo(resid.data(), sigma.data(), lpd.data(), &loo);
        if (rc != TGP_OK) { printf("loo N=%d rc=%d %s\n", N, rc, g.err.c_str()); return 1; }
        rc = g.loo(nullptr, nullptr, nullptr, nullptr);                    // the nullable outputs
        rc |= g.loo(nullptr, nullptr, nullptr, &only);
        if (rc != TGP_OK || only != loo) { printf("nullable N=%d rc=%d\n", N, rc); return 1; }
        double sum = 0.0;
        for (int i = 0; i < N; ++i) {
            if (!(sigma[i] > 0.0) || !std::isfinite(resid[i]) || !std::isfinite(lpd[i])) { printf("point %d of %d\n", i, N); return 1; }
            sum += lpd[i];
        }
        if (sum != loo) { printf("L_LOO is not the sum of lpd in index order (N=%d)\n", N); return 1; }
        printf("N=%d loo=%.12g resid0=%.6g sigma0=%.6g\n", N, loo, resid[0], sigma[0]);
    }
    printf("ok\n");
    return 0;
}
