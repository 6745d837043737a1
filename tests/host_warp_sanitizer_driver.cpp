// host_warp_sanitizer_driver.cpp -- a stand-alone program (its own main) over the host backend's input warp and its
// inverse (tgp_host::warp_points / warp_inverse; csrc/warp_math.hpp), built with -fsanitize=address,undefined by
// tests/test_warp_reference.py and run as it is: nothing is loaded into python.  It walks the grid of tests/warp_reference.py
// -- both ends of the unit interval, the smallest denormal, the neighbours of 1 -- with every output asked for and with
// none, checks the exact endpoints, the exact identity and that nothing is NaN, and calls the argument checks.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../include/turbogp.h"
#include "host_backend.hpp"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

int main() {
    const double us[] = {0.0, 5e-324, 1e-300, 1e-16, 1e-8, 0.1, 0.5, 0.9, 1.0 - 1e-8, 1.0 - ldexp(1.0, -53), 1.0};
    const double shapes[] = {0.25, 0.5, 1.0, 2.0, 4.0};
    const int64_t m = (int64_t)(sizeof us / sizeof us[0]), D = 25;
    std::vector<double> X((size_t)(m * D)), lo((size_t)D), hi((size_t)D), a((size_t)D), b((size_t)D);
    for (int64_t d = 0; d < D; ++d) {
        lo[(size_t)d] = -1.0 + 0.125 * (double)d;       // (u = (x - lo) / (hi - lo) is exact for these boxes at the ends)
        hi[(size_t)d] = lo[(size_t)d] + 2.0;
        a[(size_t)d] = shapes[d / 5];
        b[(size_t)d] = shapes[d % 5];
    }
    for (int64_t i = 0; i < m; ++i)
        for (int64_t d = 0; d < D; ++d) X[(size_t)(i * D + d)] = lo[(size_t)d] + us[i] * 2.0;
    std::string err;
    std::vector<double> w((size_t)(m * D)), du(w.size()), da(w.size()), db(w.size()), w2(w.size()), x(w.size());
    CHECK(tgp_host::warp_points(err, X.data(), m, D, lo.data(), hi.data(), a.data(), b.data(), w.data(), du.data(), da.data(), db.data()) == TGP_OK);
    CHECK(tgp_host::warp_points(err, X.data(), m, D, lo.data(), hi.data(), a.data(), b.data(), w2.data(), nullptr, nullptr, nullptr) == TGP_OK);
    CHECK(tgp_host::warp_inverse(err, w.data(), m, D, lo.data(), hi.data(), a.data(), b.data(), x.data()) == TGP_OK);
    for (int64_t i = 0; i < m; ++i)
        for (int64_t d = 0; d < D; ++d) {
            const size_t k = (size_t)(i * D + d);
            CHECK(w[k] == w2[k]);
            CHECK(w[k] >= 0.0 && w[k] <= 1.0 && !isnan(du[k]) && !isnan(da[k]) && !isnan(db[k]) && du[k] >= 0.0);
            CHECK(x[k] >= lo[(size_t)d] && x[k] <= hi[(size_t)d]);
            if (i == 0) CHECK(w[k] == 0.0 && !signbit(w[k]) && da[k] == 0.0 && db[k] == 0.0 && x[k] == lo[(size_t)d]);
            if (i == m - 1) CHECK(w[k] == 1.0 && da[k] == 0.0 && db[k] == 0.0 && x[k] == hi[(size_t)d]);
            if (a[(size_t)d] == 1.0 && b[(size_t)d] == 1.0) CHECK(w[k] == (X[k] - lo[(size_t)d]) / 2.0 && du[k] == 1.0);
        }
    // outside the box: clipped
    const double out_x[2] = {-7.0, 9.0}, one = 1.0, l0 = 0.0, h0 = 1.0;
    double out_w[2];
    CHECK(tgp_host::warp_points(err, out_x, 2, 1, &l0, &h0, &one, &one, out_w, nullptr, nullptr, nullptr) == TGP_OK);
    CHECK(out_w[0] == 0.0 && out_w[1] == 1.0);
    // the argument checks
    const double bad = 0.0, nanv = NAN;
    CHECK(tgp_host::warp_points(err, out_x, 0, 1, &l0, &h0, &one, &one, out_w, nullptr, nullptr, nullptr) == TGP_BAD_ARG);
    CHECK(tgp_host::warp_points(err, out_x, 2, 1, &h0, &l0, &one, &one, out_w, nullptr, nullptr, nullptr) == TGP_BAD_ARG);
    CHECK(tgp_host::warp_points(err, out_x, 2, 1, &l0, &h0, &bad, &one, out_w, nullptr, nullptr, nullptr) == TGP_BAD_ARG);
    CHECK(tgp_host::warp_points(err, out_x, 2, 1, &l0, &h0, &one, &nanv, out_w, nullptr, nullptr, nullptr) == TGP_BAD_ARG);
    CHECK(tgp_host::warp_points(err, nullptr, 2, 1, &l0, &h0, &one, &one, out_w, nullptr, nullptr, nullptr) == TGP_BAD_ARG);
    CHECK(tgp_host::warp_inverse(err, out_w, 2, 1, &l0, &l0, &one, &one, out_w) == TGP_BAD_ARG);
    CHECK(tgp_host::warp_inverse(err, out_w, 2, 0, &l0, &h0, &one, &one, out_w) == TGP_BAD_ARG);
    CHECK(!err.empty());
    printf("ok\n");
    return 0;
}
