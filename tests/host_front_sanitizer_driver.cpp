// Stand-alone walk of csrc/host_front.hpp (the Pareto front of tgp_ehvi_set_front) for AddressSanitizer + UBSan: its own
// main, nothing loaded into python.  tests/test_ehvi_abi.py compiles it with -fsanitize=address,undefined and runs it.
// Inputs: duplicates, ties in one coordinate, points on the reference's boundary, every point dropped, n = 0, all four
// sign pairs, and n = 5000 with a front of exactly 256 and of 257.  Prints "ok" last; any mismatch is exit code 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "host_front.hpp"

using tgp_front::Front;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static bool same(const Front &f, const std::vector<double> &want) {
    if (f.u.size() * 2 != want.size()) return false;
    for (size_t i = 0; i < f.u.size(); ++i)
        if (f.u[i].first != want[2 * i] || f.u[i].second != want[2 * i + 1]) return false;
    return true;
}

// n points of which exactly `front` are non-dominated: a staircase, and below it points that each stair dominates
static std::vector<double> staircase(int n, int front) {
    std::vector<double> Y;
    Y.reserve((size_t)(2 * n));
    unsigned long long s = 12345;
    auto next = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; };
    for (int i = 0; i < n; ++i) {
        const int k = i % front;
        const double u1 = 1.0 + k, u2 = (double)front - k;
        if (i < front) { Y.push_back(u1); Y.push_back(u2); }
        else { Y.push_back(u1 - 0.9 * next()); Y.push_back(u2 - 0.9 * next() - 1e-9); }
    }
    // (shuffle: the builder may not rely on the order)
    for (int i = n - 1; i > 0; --i) {
        const int j = (int)(next() * (i + 1));
        std::swap(Y[2 * i], Y[2 * j]);
        std::swap(Y[2 * i + 1], Y[2 * j + 1]);
    }
    return Y;
}

int main() {
    const double ref0[2] = {0.0, 0.0};
    Front f;
    {   // duplicates, ties in one coordinate, the boundary
        const double Y[] = {1, 3, 1, 3, 2, 2, 2, 1.5, 1.5, 2, 3, 1, 0, 5, 5, 0, 0.5, 0.5};
        CHECK(tgp_front::build_front(Y, 9, 1.0, 1.0, ref0, 256, f) == tgp_front::FRONT_OK);
        CHECK(same(f, {1, 3, 2, 2, 3, 1}));
        CHECK(f.hv == 6.0);
        std::vector<double> a, c;
        tgp_front::front_strips(f, a, c);
        CHECK(a.size() == 4 && c.size() == 4 && a[0] == 0.0 && a[3] == 3.0 && c[0] == 3.0 && c[3] == 0.0);
    }
    {   // every point dropped; n = 0 with and without a pointer
        const double Y[] = {0, 1, -1, -1};
        CHECK(tgp_front::build_front(Y, 2, 1.0, 1.0, ref0, 256, f) == tgp_front::FRONT_OK && f.size() == 0 && f.hv == 0.0);
        CHECK(tgp_front::build_front(nullptr, 0, 1.0, 1.0, ref0, 256, f) == tgp_front::FRONT_OK && f.size() == 0);
        CHECK(tgp_front::build_front(Y, 0, 1.0, 1.0, ref0, 256, f) == tgp_front::FRONT_OK && f.size() == 0);
        std::vector<double> a, c;
        tgp_front::front_strips(f, a, c);
        CHECK(a.size() == 1 && c.size() == 1);
    }
    for (int s1 = -1; s1 <= 1; s1 += 2)     // all four sign pairs: the same oriented front
        for (int s2 = -1; s2 <= 1; s2 += 2) {
            const double base[] = {1, 3, 2, 2, 3, 1, 1.5, 1.5};
            double Y[8];
            for (int i = 0; i < 4; ++i) { Y[2 * i] = s1 * base[2 * i]; Y[2 * i + 1] = s2 * base[2 * i + 1]; }
            CHECK(tgp_front::build_front(Y, 4, s1, s2, ref0, 256, f) == tgp_front::FRONT_OK);
            CHECK(same(f, {1, 3, 2, 2, 3, 1}) && f.hv == 6.0 && f.sf[0] == s1 && f.sf[1] == s2);
        }
    {   // refusals leave the output untouched
        const double Y[] = {1, 3, 2, 2};
        CHECK(tgp_front::build_front(Y, 2, 1.0, 1.0, ref0, 256, f) == tgp_front::FRONT_OK && f.size() == 2);
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        const double Yn[] = {1, nan}, Yi[] = {inf, 1}, rn[2] = {0.0, nan};
        CHECK(tgp_front::build_front(Yn, 1, 1.0, 1.0, ref0, 256, f) == tgp_front::FRONT_BAD_Y);
        CHECK(tgp_front::build_front(Yi, 1, 1.0, 1.0, ref0, 256, f) == tgp_front::FRONT_BAD_Y);
        CHECK(tgp_front::build_front(Y, 2, 1.0, 1.0, rn, 256, f) == tgp_front::FRONT_BAD_REF);
        CHECK(tgp_front::build_front(Y, 2, 1.0, 1.0, nullptr, 256, f) == tgp_front::FRONT_BAD_REF);
        CHECK(tgp_front::build_front(Y, 2, 0.5, 1.0, ref0, 256, f) == tgp_front::FRONT_BAD_SF);
        CHECK(tgp_front::build_front(Y, 2, 1.0, 0.0, ref0, 256, f) == tgp_front::FRONT_BAD_SF);
        CHECK(tgp_front::build_front(nullptr, 2, 1.0, 1.0, ref0, 256, f) == tgp_front::FRONT_BAD_Y);
        CHECK(tgp_front::build_front(Y, -1, 1.0, 1.0, ref0, 256, f) == tgp_front::FRONT_BAD_Y);
        CHECK(f.size() == 2);
    }
    {   // n = 5000: a front of exactly 256 is taken, one of 257 refused (and the previous one kept)
        const std::vector<double> Y = staircase(5000, 256);
        CHECK(tgp_front::build_front(Y.data(), 5000, 1.0, 1.0, ref0, 256, f) == tgp_front::FRONT_OK);
        CHECK(f.size() == 256);
        bool sorted = true;
        for (size_t i = 1; i < f.u.size(); ++i) sorted = sorted && f.u[i].first > f.u[i - 1].first && f.u[i].second < f.u[i - 1].second;
        CHECK(sorted);
        double hv = 0.0;
        for (int k = 0; k < 256; ++k) hv += 256.0 - k;
        CHECK(f.hv == hv);
        const std::vector<double> Z = staircase(5000, 257);
        CHECK(tgp_front::build_front(Z.data(), 5000, 1.0, 1.0, ref0, 256, f) == tgp_front::FRONT_TOO_LARGE);
        CHECK(f.size() == 256);
        CHECK(tgp_front::build_front(Z.data(), 5000, 1.0, 1.0, ref0, 257, f) == tgp_front::FRONT_OK && f.size() == 257);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
