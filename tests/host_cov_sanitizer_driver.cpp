// Driver of tests/test_cov_abi.py::test_host_backend_joint_posterior_under_sanitizers: the host backend's joint
// posterior (turbo_amd/csrc/host_backend.cpp: predict_cov, sample_joint) on a 6-point model, compiled with
// -fsanitize=address,undefined.  A stand-alone program: CPU build only, never run on a GPU machine.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/turbogp.h"
#include "host_backend.hpp"

int main() {
    const int N = 6, D = 2;
    std::vector<double> X(N * D), y(N), ls(D, 0.5);
    unsigned s = 77u;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; };
    for (auto &v : X) v = rnd();
    for (int i = 0; i < N; ++i) y[i] = std::sin(3 * X[i * D]) + X[i * D + 1];
    tgp_host::HostGP g;
    double lml, ym, ys;
    int rc = g.fit(X.data(), N, D, y.data(), TGP_MATERN52, 1.1, ls.data(), D, 1e-3, 1e-10, 1, &lml, &ym, &ys);
    if (rc != TGP_OK) { printf("fit rc=%d\n", rc); return 1; }
    for (int m : {1, 5, 17}) {
        const int S = 3;
        std::vector<double> Xq(m * D), mu(m), cov(m * m), eps(S * m), yo(S * m), eo(S * m);
        for (auto &v : Xq) v = rnd();
        for (auto &v : eps) v = rnd() - 0.5;
        int64_t neg = -1;
        for (int latent = 0; latent < 2; ++latent) {
            rc = g.predict_cov(Xq.data(), m, latent, mu.data(), cov.data(), &neg);
            if (rc != TGP_OK || neg < 0) { printf("predict_cov m=%d rc=%d\n", m, rc); return 1; }
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < i; ++j)
                    if (cov[i * m + j] != cov[j * m + i]) { printf("asymmetric\n"); return 1; }
            rc = g.sample_joint(Xq.data(), m, S, latent, 1e-8, eps.data(), yo.data(), eo.data(), mu.data());
            if (rc != TGP_OK) { printf("sample_joint m=%d rc=%d %s\n", m, rc, g.err.c_str()); return 1; }
        }
        rc = g.predict_cov(Xq.data(), m, 0, nullptr, cov.data(), nullptr);           // the nullable outputs
        rc |= g.sample_joint(Xq.data(), m, S, 0, 0.0, eps.data(), yo.data(), nullptr, nullptr);
        if (rc != TGP_OK) { printf("nullable m=%d rc=%d\n", m, rc); return 1; }
        if (g.sample_joint(Xq.data(), m, S, 0, 0.0, nullptr, yo.data(), nullptr, nullptr) != TGP_BAD_ARG) { printf("eps_in NULL accepted\n"); return 1; }
        printf("m=%d mu0=%.6f cov00=%.6g y00=%.6f\n", m, mu[0], cov[0], yo[0]);
    }
    // duplicated rows of the latent function without a nugget: the pivot rule refuses
    std::vector<double> dup = {0.3, 0.4, 0.3, 0.4}, e2(2, 0.0), y2(2);
    if (g.sample_joint(dup.data(), 2, 1, 1, 0.0, e2.data(), y2.data(), nullptr, nullptr) != TGP_NOT_PD) { printf("duplicate accepted\n"); return 1; }
    if (g.sample_joint(dup.data(), 2, 1, 1, 1e-6, e2.data(), y2.data(), nullptr, nullptr) != TGP_OK) { printf("nugget refused\n"); return 1; }
    printf("ok\n");
    return 0;
}
