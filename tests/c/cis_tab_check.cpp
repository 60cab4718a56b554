// Host check of grape_cis::cis_tab (robustgrape_amd/csrc/grape_cis.hpp, the merged walks' e^{i t}) and its table
// against x87 long double sinl / cosl.  Prints the largest absolute error in units of 2^-52 over: a dense uniform
// grid on [-4 pi, 4 pi]; log-spaced magnitudes of both signs up to the fast-path bound; random arguments that land
// on every table index; arguments within 1e-12 of every k pi / 64 (the switch between table entries), around the
// origin and near the bound.  Then the values at exact points, how many table indices the sweep met, and the
// largest distance of a table entry from the long double value in units of its own last place.
#include "grape_cis.hpp"

#include <cmath>
#include <cstdio>
#include <random>

int main() {
    using namespace grape_cis;
    double worst_s = 0, worst_c = 0;
    bool seen[kCisTabN] = {};
    const long double kUnit = 2.220446049250313e-16L, kPi = 3.141592653589793238462643383279502884L;
    auto k = [](int i) { return kCisCoef[i]; };
    auto probe = [&](double t) {
        if (std::fabs(t) > kCisTabFast) return;
        double s, c;
        cis_tab(t, kCisTable, s, c, k);
        worst_s = std::fmax(worst_s, (double)(fabsl((long double)s - sinl((long double)t)) / kUnit));
        worst_c = std::fmax(worst_c, (double)(fabsl((long double)c - cosl((long double)t)) / kUnit));
        seen[(int)std::rint(t * kCisCoef[kTabInv_]) & (kCisTabN - 1)] = true;
    };
    const double four_pi = (double)(4 * kPi);
    const int dense = 1000000;
    for (int i = 0; i <= dense; ++i) probe(-four_pi + 2 * four_pi * i / dense);
    const int logn = 500000;  // 1e-8 .. kCisTabFast, both signs
    const double l0 = std::log(1.0e-8), l1 = std::log(kCisTabFast);
    for (int i = 0; i <= logn; ++i) {
        const double m = std::fmin(std::exp(l0 + (l1 - l0) * i / logn), kCisTabFast);
        probe(m);
        probe(-m);
    }
    std::mt19937_64 g(1);
    for (int i = 0; i < 500000; ++i) probe(std::uniform_real_distribution<double>(-kCisTabFast, kCisTabFast)(g));
    // the edges between table entries sit at odd multiples of pi / 128; the entries themselves at k pi / 64
    const long kmax = (long)(kCisTabFast * 64 / (double)kPi);
    auto around = [&](long double x) {
        for (int j = -4; j <= 4; ++j) probe((double)(x + j * 0.25e-12L));
        probe(std::nextafter((double)x, 1e9));
        probe(std::nextafter((double)x, -1e9));
    };
    for (long kk = -4 * kCisTabN; kk <= 4 * kCisTabN; ++kk) {
        around(kk * kPi / 64);
        around((2 * kk + 1) * kPi / 128);
    }
    for (long kk = -kmax; kk <= kmax; ++kk) {  // every k pi / 64 below the bound
        const long double x = kk * kPi / 64;
        probe((double)x);
        probe((double)(x + 0.5e-12L));
        probe((double)(x - 0.5e-12L));
    }
    for (long kk = kmax - 2 * kCisTabN; kk <= kmax; ++kk) {
        around(kk * kPi / 64);
        around(-kk * kPi / 64);
        around((2 * kk - 1) * kPi / 128);
    }
    probe(kCisTabFast);
    probe(-kCisTabFast);
    int nseen = 0;
    for (bool b : seen) nseen += b;
    double tab_ulp = 0;  // |entry - exact| in units of the entry's own last place (0 for the exact entries)
    int exact_axes = 1;
    for (int j = 0; j < kCisTabN; ++j) {
        const long double a = 2 * kPi * j / kCisTabN;
        const double v[2] = {kCisTable[j].c, kCisTable[j].s};
        const long double ref[2] = {cosl(a), sinl(a)};
        for (int m = 0; m < 2; ++m) {
            if (j % (kCisTabN / 4) == 0) {  // multiples of pi / 2: exactly 0 and +-1
                const double want = (double)std::lround((double)ref[m]);
                exact_axes = exact_axes && v[m] == want;
                continue;
            }
            const double ulp = std::nextafter(std::fabs(v[m]), 2.0) - std::fabs(v[m]);
            tab_ulp = std::fmax(tab_ulp, (double)(fabsl((long double)v[m] - ref[m]) / ulp));
        }
    }
    double s0, c0;
    cis_tab(0.0, kCisTable, s0, c0, k);
    printf("sin_err %.4f\ncos_err %.4f\nsin0 %.17g\ncos0 %.17g\nindices %d\ntable_ulp %.4f\ntable_axes_exact %d\n", worst_s,
           worst_c, s0, c0, nseen, tab_ulp, exact_axes);
    return 0;
}
