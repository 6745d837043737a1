// host_front.hpp -- the Pareto front of tgp_ehvi_set_front (include/turbogp.h, "two-objective expected hypervolume
// improvement") as plain C++: no HIP header, O(n log n), so that a stand-alone program can walk it
// (tests/host_front_sanitizer_driver.cpp).
//
// In the oriented coordinates u_j = sf_j y_j with the reference point r = (sf_1 ref_1, sf_2 ref_2):
//   1. drop every pair that does not strictly beat r in both coordinates;
//   2. sort by u_1 descending, u_2 descending among equal u_1 (duplicates become neighbours);
//   3. walk once and keep a pair only where its u_2 exceeds every u_2 kept so far: weak dominance removes a point, equal
//      u_1 keeps the larger u_2, duplicates merge;
//   4. reverse: u_1 strictly ascending, u_2 strictly descending.
// The dominated area over r is the sum of the strips (u_1^(i) - u_1^(i-1)) (u_2^(i) - r_2), u_1^(0) = r_1, in that order.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

namespace tgp_front {

struct Front {
    double sf[2] = {1.0, 1.0};
    double r[2] = {0.0, 0.0};                       // oriented reference point
    std::vector<std::pair<double, double>> u;       // oriented, sorted
    double hv = 0.0;
    int64_t size() const { return (int64_t)u.size(); }
};

enum Status { FRONT_OK = 0, FRONT_BAD_SF, FRONT_BAD_REF, FRONT_BAD_Y, FRONT_TOO_LARGE };

// Y (n, 2) raw pairs (may be null when n == 0), ref 2 raw values; out is written only on FRONT_OK
inline Status build_front(const double *Y, int64_t n, double sf1, double sf2, const double *ref, int64_t max_front, Front &out) {
    if ((sf1 != 1.0 && sf1 != -1.0) || (sf2 != 1.0 && sf2 != -1.0)) return FRONT_BAD_SF;
    if (!ref || !std::isfinite(ref[0]) || !std::isfinite(ref[1])) return FRONT_BAD_REF;
    if (n < 0 || (n > 0 && !Y)) return FRONT_BAD_Y;
    for (int64_t e = 0; e < 2 * n; ++e)
        if (!std::isfinite(Y[e])) return FRONT_BAD_Y;
    const double r1 = sf1 * ref[0], r2 = sf2 * ref[1];
    std::vector<std::pair<double, double>> pts;
    pts.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const double u1 = sf1 * Y[2 * i], u2 = sf2 * Y[2 * i + 1];
        if (u1 > r1 && u2 > r2) pts.emplace_back(u1, u2);
    }
    std::sort(pts.begin(), pts.end(), [](const std::pair<double, double> &a, const std::pair<double, double> &b) {
        return a.first > b.first || (a.first == b.first && a.second > b.second);
    });
    std::vector<std::pair<double, double>> keep;
    double top = r2;
    for (const auto &p : pts)
        if (p.second > top) {
            keep.push_back(p);
            top = p.second;
        }
    if ((int64_t)keep.size() > max_front) return FRONT_TOO_LARGE;
    std::reverse(keep.begin(), keep.end());
    double hv = 0.0, left = r1;
    for (const auto &p : keep) {
        hv += (p.first - left) * (p.second - r2);
        left = p.first;
    }
    out.sf[0] = sf1; out.sf[1] = sf2;
    out.r[0] = r1; out.r[1] = r2;
    out.u = std::move(keep);
    out.hv = hv;
    return FRONT_OK;
}

// the P + 1 strips' breakpoints a_0 .. a_P (a_{P+1} = +inf is implied) and levels c_0 .. c_P
inline void front_strips(const Front &f, std::vector<double> &a, std::vector<double> &c) {
    const size_t P = f.u.size();
    a.assign(P + 1, 0.0);
    c.assign(P + 1, 0.0);
    a[0] = f.r[0];
    for (size_t i = 1; i <= P; ++i) a[i] = f.u[i - 1].first;
    for (size_t i = 0; i < P; ++i) c[i] = f.u[i].second;
    c[P] = f.r[1];
}

}  // namespace tgp_front
