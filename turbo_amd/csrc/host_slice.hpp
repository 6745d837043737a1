// host_slice.hpp -- the hyper-parameter MCMC of tgp_hyper_sample as plain host C++: coordinate-wise slice sampling
// with stepping-out and shrinkage (Neal, "Slice sampling", Ann. Statist. 2003, figs. 3 and 5) of
//     p(theta) ~ exp(LML(theta))  on the box [log_lo, log_hi],
// i.e. a uniform prior in log space over the bounds the optimiser uses.  It is the 'marginalise' way of handling the
// hyper-parameters that the author's older library names and leaves #TODO (old_library/bayesian_optimiser.py:53-75,
// :153-165; the integrated acquisition of Snoek et al. 2012).  The objective is a callable -- tgp_fit on the caller's
// handle, taken for its LML -- so there is no interpreter between two evaluations, as in host_lbfgsb.hpp.
//
// Randomness is counter-based: the j-th uniform of a call is philox_u53 of words 0 and 1 of
//     philox4x32_10(j lo, j hi, SLICE_TAG, 0, seed lo, seed hi),
// the host twin of csrc/philox.hpp restated below (that header is __device__ only), so a walk is a pure function of
// the inputs.  Consumption order, per update of one free coordinate p at the current point x with value f = LML(x):
//     1. u  -> the slice level  f + log(u)
//     2. v  -> the interval's position:  L = x[p] - width[p] v,  R = L + width[p]
//        stepping out: at most SLICE_STEPS moves of width[p] per side, the left side first, each move made while the end
//        point lies inside the box and LML(end point) > level; an end that leaves the box is clipped to the bound
//        (no evaluation there: the density is zero outside) and the side is finished
//     3. one uniform t per shrinkage proposal  x1 = L + t (R - L):  accepted when LML(x1) > level, else the interval
//        shrinks to x1 on x[p]'s side of it
// One sweep is one pass over the free coordinates in index order; an entry with log_lo == log_hi is fixed at the
// bound and never sampled.  `burn` sweeps are discarded; sample k (k = 0 .. S-1) is the state after sweep
// burn + (k + 1) thin.
#pragma once
#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/turbogp.h"

namespace tgp {

constexpr uint32_t SLICE_TAG = 0x534C4943u;   // "SLIC"
constexpr int SLICE_STEPS = 8;                // stepping-out moves per side
constexpr int SLICE_SHRINKS = 1000;           // shrinkage proposals per update (never reached in exact arithmetic: the interval collapses onto x)

// csrc/philox.hpp's round function and 53-bit uniform on the host (tests/philox_ref.py is the NumPy twin)
inline void host_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
inline double host_philox_u53(uint32_t a, uint32_t b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

struct SliceStream {
    uint64_t seed, j = 0;
    explicit SliceStream(uint64_t s) : seed(s) {}
    double next() {
        uint32_t r[4];
        host_philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), SLICE_TAG, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
        ++j;
        return host_philox_u53(r[0], r[1]);
    }
};

// status codes of `eval`: 0 = ok (lml set), 1 = not positive definite (TGP_NOT_PD), anything else = an error to hand back
constexpr int SLICE_OK = 0, SLICE_NOT_PD = 1;

// eval(theta (P), &lml) -> status.  Returns 0, or the first status that is neither ok nor "not PD" -- and "not PD"
// itself when theta0 is (a proposal that is not PD counts as LML = -inf: rejected, counted in not_pd).
// theta0's free entries must lie inside the box (the caller checks).  theta_out (S, P), lml_out (S).
template <class Eval>
int slice_sample(Eval &&eval, int P, const double *theta0, const double *lo, const double *hi, const double *width,
                 int64_t S, int64_t burn, int64_t thin, uint64_t seed, double *theta_out, double *lml_out,
                 int64_t *evaluations, int64_t *not_pd) {
    std::vector<double> x((size_t)P), xt((size_t)P);
    for (int p = 0; p < P; ++p) x[(size_t)p] = lo[p] < hi[p] ? theta0[p] : lo[p];
    int64_t evals = 0, npd = 0;
    int err = SLICE_OK;
    // LML with coordinate p moved to v; -inf where the matrix is not PD
    auto value_at = [&](int p, double v) -> double {
        xt = x;
        xt[(size_t)p] = v;
        double f = -INFINITY;
        const int rc = eval(xt.data(), &f);
        ++evals;
        if (rc == SLICE_NOT_PD) { ++npd; return -INFINITY; }
        if (rc != SLICE_OK) { if (err == SLICE_OK) err = rc; return -INFINITY; }
        return f;
    };
    double f = 0.0;
    {
        const int rc = eval(x.data(), &f);
        ++evals;
        if (evaluations) *evaluations = evals;
        if (not_pd) *not_pd = 0;
        if (rc != SLICE_OK) return rc;
    }
    SliceStream rng(seed);
    const int64_t sweeps = burn + S * thin;
    int64_t kept = 0;
    for (int64_t sw = 1; sw <= sweeps && err == SLICE_OK; ++sw) {
        for (int p = 0; p < P && err == SLICE_OK; ++p) {
            if (!(lo[p] < hi[p])) continue;
            const double w = width ? width[p] : 1.0;
            const double level = f + log(rng.next());
            double L = x[(size_t)p] - w * rng.next();
            double R = L + w;
            for (int j = 0; j < SLICE_STEPS && err == SLICE_OK; ++j) {
                if (L <= lo[p]) break;
                if (!(value_at(p, L) > level)) break;
                L -= w;
            }
            if (L < lo[p]) L = lo[p];
            for (int j = 0; j < SLICE_STEPS && err == SLICE_OK; ++j) {
                if (R >= hi[p]) break;
                if (!(value_at(p, R) > level)) break;
                R += w;
            }
            if (R > hi[p]) R = hi[p];
            for (int j = 0; j < SLICE_SHRINKS && err == SLICE_OK; ++j) {
                const double x1 = L + rng.next() * (R - L);
                const double f1 = value_at(p, x1);
                if (f1 > level) { x[(size_t)p] = x1; f = f1; break; }
                if (x1 < x[(size_t)p]) L = x1; else R = x1;
            }
        }
        if (err == SLICE_OK && sw > burn && (sw - burn) % thin == 0) {
            for (int p = 0; p < P; ++p) theta_out[kept * P + p] = x[(size_t)p];
            lml_out[kept] = f;
            ++kept;
        }
    }
    if (evaluations) *evaluations = evals;
    if (not_pd) *not_pd = npd;
    return err;
}

// the argument rules of tgp_hyper_sample, shared by both libraries; returns a message or nullptr
inline const char *slice_check_args(const double *X, int64_t N, int64_t D, const double *y, int kernel, const double *theta0,
                                    int64_t n_ls, const double *log_lo, const double *log_hi, double jitter, int64_t S,
                                    int64_t burn, int64_t thin, const double *width, const double *theta_out,
                                    const double *lml_out) {
    if (!X || !y || !theta0 || !log_lo || !log_hi || !theta_out || !lml_out)
        return "need X, y, theta0, log_lo, log_hi, theta_out, lml_out";
    if (kernel < 0 || kernel > 3) return "unknown kernel";
    if (N < 1 || D < 1 || D > 4096 || (n_ls != 1 && n_ls != D)) return "needs N >= 1, 1 <= D <= 4096, n_ls 1 or D";
    if (S < 1 || S > 64 || burn < 0 || thin < 1) return "needs 1 <= S <= 64, burn >= 0, thin >= 1";
    if (!(jitter >= 0.0)) return "jitter >= 0 required";
    const int64_t P = 2 + n_ls;
    for (int64_t i = 0; i < P; ++i) {
        if (i == P - 1 && log_lo[i] == -INFINITY && log_hi[i] == -INFINITY) continue;   // no noise term
        if (!(log_lo[i] <= log_hi[i]) || !isfinite(log_lo[i]) || !isfinite(log_hi[i]))
            return "bounds must be finite with lo <= hi (the noise entry may be fixed at -inf: no noise term)";
        if (log_lo[i] < log_hi[i] && !(theta0[i] >= log_lo[i] && theta0[i] <= log_hi[i])) return "theta0 must lie inside the box";
        if (width && log_lo[i] < log_hi[i] && !(width[i] > 0.0 && isfinite(width[i]))) return "widths must be finite and > 0";
    }
    return nullptr;
}

// theta (P) -> the arguments of tgp_fit
inline void slice_unpack(const double *theta, int64_t n_ls, double &constant, double *ls, double &noise) {
    constant = exp(theta[0]);
    for (int64_t d = 0; d < n_ls; ++d) ls[d] = exp(theta[1 + d]);
    noise = exp(theta[1 + n_ls]);
}

static_assert(SLICE_OK == TGP_OK && SLICE_NOT_PD == TGP_NOT_PD, "host_slice.hpp's statuses are tgp_status values");

// tgp_hyper_sample itself, for both libraries: the argument rules, the walk and the texts.  Every evaluation is
// fit(constant, ls, noise, &lml) -> tgp_status: the handle's own tgp_fit, taken for its LML.  err: the handle's message
// (a fit that fails has left its own there).
template <class Fit>
int hyper_sample(Fit &&fit, std::string &err, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                 const double *theta0, int64_t n_ls, const double *log_lo, const double *log_hi, double jitter, int64_t S,
                 int64_t burn, int64_t thin, const double *width, uint64_t seed, double *theta_out, double *lml_out,
                 int64_t *evaluations, int64_t *not_pd) {
    if (const char *msg = slice_check_args(X, N, D, y, kernel, theta0, n_ls, log_lo, log_hi, jitter, S, burn, thin, width,
                                           theta_out, lml_out)) {
        err = std::string("tgp_hyper_sample: ") + msg;
        return TGP_BAD_ARG;
    }
    std::vector<double> ls((size_t)n_ls);
    auto eval = [&](const double *theta, double *lml) {
        double constant, noise;
        slice_unpack(theta, n_ls, constant, ls.data(), noise);
        return fit(constant, ls.data(), noise, lml);
    };
    const int rc = slice_sample(eval, (int)(2 + n_ls), theta0, log_lo, log_hi, width, S, burn, thin, seed, theta_out, lml_out,
                                evaluations, not_pd);
    if (rc != TGP_OK) err = "tgp_hyper_sample: " + std::string(rc == TGP_NOT_PD ? "at theta0: " : "") + err;
    return rc;
}

}  // namespace tgp
