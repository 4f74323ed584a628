// Contamination and sample identity from the base counts of a pileup at sites (include/hello_mi355x.h:
// hello_contam_*): the error rate, the likelihood of a two-sample mixture on a grid of mixing fractions with its interval, and the
// log odds that two BAMs hold one person.  Plain C++17 -- no HIP, no device -- so it also builds into a stand-alone host program
// (tests/abi/contam_check.cpp).  hello_amd/contamination.py restates every formula in NumPy.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

namespace hello {
namespace {

constexpr int kContamGrid = 501;                 // alpha_k = k / 1000, k = 0 .. 500
constexpr double kContamDrop = 1.92;             // the interval: LL_k >= LL_max - 1.92
constexpr double kContamMinError = 1e-4, kContamMaxError = 0.1;
constexpr int kContamMaxThreads = 8;

// clamp(1.5 * sum(o) / sum(r + a + o)): errors are uniform over three bases and two of them show as `o`.
inline double contam_error_rate(const int64_t* r, const int64_t* a, const int64_t* o, int64_t n) {
    double wrong = 0.0, all = 0.0;               // sums of integers below 2^53: exact
    for (int64_t i = 0; i < n; ++i) {
        wrong += (double)o[i];
        all += (double)r[i] + (double)a[i] + (double)o[i];
    }
    if (all <= 0.0) return kContamMinError;
    return std::min(std::max(1.5 * wrong / all, kContamMinError), kContamMaxError);
}

// A read's probability of showing ALT / REF over a genotype of g ALT copies.
inline double contam_p_alt(int g, double e) { return (g / 2.0) * (1.0 - e) + (1.0 - g / 2.0) * e / 3.0; }
inline double contam_p_ref(int g, double e) { return (1.0 - g / 2.0) * (1.0 - e) + (g / 2.0) * e / 3.0; }

inline void contam_log_prior(double af, double* lp) {             // Hardy-Weinberg, log
    lp[0] = 2.0 * std::log(1.0 - af);
    lp[1] = std::log(2.0) + std::log(af) + std::log(1.0 - af);
    lp[2] = 2.0 * std::log(af);
}

template <int N> inline double contam_lse(const double* x) {
    double m = x[0];
    for (int i = 1; i < N; ++i) m = std::max(m, x[i]);
    double s = 0.0;
    for (int i = 0; i < N; ++i) s += std::exp(x[i] - m);
    return m + std::log(s);
}

// LL[k] of one grid point: the log terms of the nine genotype pairs first, then the sites in their order.
inline double contam_grid_point(int k, double e, const int64_t* r, const int64_t* a, const double* lp, int64_t n) {
    const double alpha = k / 1000.0;
    double lq_ref[9], lq_alt[9];
    for (int g1 = 0; g1 < 3; ++g1)
        for (int g2 = 0; g2 < 3; ++g2) {
            lq_ref[g1 * 3 + g2] = std::log((1.0 - alpha) * contam_p_ref(g1, e) + alpha * contam_p_ref(g2, e));
            lq_alt[g1 * 3 + g2] = std::log((1.0 - alpha) * contam_p_alt(g1, e) + alpha * contam_p_alt(g2, e));
        }
    double ll = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (r[i] + a[i] <= 0) continue;
        double x[9];
        for (int g1 = 0; g1 < 3; ++g1)
            for (int g2 = 0; g2 < 3; ++g2)
                x[g1 * 3 + g2] = lp[3 * i + g1] + lp[3 * i + g2] + (double)r[i] * lq_ref[g1 * 3 + g2] + (double)a[i] * lq_alt[g1 * 3 + g2];
        ll += contam_lse<9>(x);
    }
    return ll;
}

// out[HELLO_CONTAM_OUT]: the error rate, k of the greatest LL (the smallest at a tie), the interval's k_lo and k_hi, LL[501].  The
// grid points are dealt to host threads; every point sums its sites in their order, so no number depends on the thread count.
inline void contam_estimate(const int64_t* r, const int64_t* a, const int64_t* o, const double* af, int64_t n, double* out,
                            int threads = 0) {
    const double e = contam_error_rate(r, a, o, n);
    std::vector<double> lp((size_t)n * 3);
    for (int64_t i = 0; i < n; ++i) contam_log_prior(af[i], lp.data() + 3 * i);
    double* ll = out + 4;
    if (threads <= 0) threads = n * kContamGrid < (int64_t)1 << 16 ? 1 : std::min<int>(kContamMaxThreads, std::max(1u, std::thread::hardware_concurrency()));
    auto work = [&](int first) {
        for (int k = first; k < kContamGrid; k += threads) ll[k] = contam_grid_point(k, e, r, a, lp.data(), n);
    };
    if (threads == 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (int t = 1; t < threads; ++t) pool.emplace_back(work, t);
        work(0);
        for (std::thread& t : pool) t.join();
    }
    int best = 0;
    for (int k = 1; k < kContamGrid; ++k)
        if (ll[k] > ll[best]) best = k;
    int lo = best, hi = best;
    for (int k = 0; k < kContamGrid; ++k)
        if (ll[k] >= ll[best] - kContamDrop) { lo = k; break; }
    for (int k = kContamGrid - 1; k >= 0; --k)
        if (ll[k] >= ll[best] - kContamDrop) { hi = k; break; }
    out[0] = e;
    out[1] = best;
    out[2] = lo;
    out[3] = hi;
}

// out[2]: the log odds of "one person" against "two unrelated people" over the sites with r + a > 0 in both BAMs, each BAM at its
// own error rate; and the number of those sites.
inline void contam_identity(const int64_t* r1, const int64_t* a1, const int64_t* o1, const int64_t* r2, const int64_t* a2,
                            const int64_t* o2, const double* af, int64_t n, double* out) {
    const double e1 = contam_error_rate(r1, a1, o1, n), e2 = contam_error_rate(r2, a2, o2, n);
    double lr1[3], la1[3], lr2[3], la2[3];
    for (int g = 0; g < 3; ++g) {
        lr1[g] = std::log(contam_p_ref(g, e1));
        la1[g] = std::log(contam_p_alt(g, e1));
        lr2[g] = std::log(contam_p_ref(g, e2));
        la2[g] = std::log(contam_p_alt(g, e2));
    }
    double lod = 0.0;
    int64_t used = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (r1[i] + a1[i] <= 0 || r2[i] + a2[i] <= 0) continue;
        double lp[3], both[3], one[3], two[3];
        contam_log_prior(af[i], lp);
        for (int g = 0; g < 3; ++g) {
            const double l1 = (double)r1[i] * lr1[g] + (double)a1[i] * la1[g], l2 = (double)r2[i] * lr2[g] + (double)a2[i] * la2[g];
            both[g] = lp[g] + l1 + l2;
            one[g] = lp[g] + l1;
            two[g] = lp[g] + l2;
        }
        lod += contam_lse<3>(both) - contam_lse<3>(one) - contam_lse<3>(two);
        ++used;
    }
    out[0] = lod;
    out[1] = (double)used;
}

}  // namespace
}  // namespace hello
