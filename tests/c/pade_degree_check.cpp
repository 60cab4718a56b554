// Host check of the small engine's degree choice (robustgrape_amd/csrc/grape_pade_degree.hpp pade_degree: the
// lines k_expm, k_expm_high and k_expm_raw run on the device) against a plain restatement in x87 long double
// (64-bit mantissa): m from Julia's thresholds, s the smallest count >= 0 with q <= 2^s, q = nA / 5.4 as the
// double the rule divides to, found by counting up (2^s is exact there for every s a double can ask for).
// The rule takes ceil(log2(q)) in double: where q lies a few ulps above 2^k, log2(q) rounds to k itself and the
// rule returns k, one below the count (from k = 4 the upper neighbour of 5.4 2^k is such a norm).  Julia's
// expression has the same rounding and the rule keeps it bit for bit, so that one outcome is accepted where
// log2l(q) - k is within one double ulp of k, and counted apart (log2_rounded); anything else is a mismatch.
// Inputs: 0, denormals, 1e-300; the five thresholds and their neighbouring doubles; 5.4 2^s and its upper
// neighbour for s = 1 .. 60; 1e300 and DBL_MAX; a log-spaced sweep of a million norms over the whole range of
// the format; +inf and NaN, which must return m = 13, s = 0.  Prints the counts, then m and s of every norm
// given on the command line (hexadecimal floats), for the caller to compare with the oracle's degree choice.
#include "grape_pade_degree.hpp"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

static int ref_degree(double nA, int &s) {
    s = 0;
    const long double v = nA, t3 = 0.015, t5 = 0.25, t7 = 0.95, t9 = 2.1;  // the rule's doubles, widened
    if (v <= t3) return 3;
    if (v <= t5) return 5;
    if (v <= t7) return 7;
    if (v <= t9) return 9;
    const long double q = (long double)(nA / 5.4);
    while (s < 1200 && q > scalbnl(1.0L, s)) ++s;
    return 13;
}

int main(int argc, char **argv) {
    using grape::pade_degree;
    long checked = 0, bad = 0, rounded = 0;
    int smax = 0;
    double first_bad = 0.0;
    auto probe = [&](double nA) {
        int s = -1, sr = -1;
        const int m = pade_degree(nA, s), mr = ref_degree(nA, sr);
        ++checked;
        if (s > smax) smax = s;
        if (m == mr && s == sr) return;
        if (m == mr && s == sr - 1) {
            const long double excess = log2l((long double)(nA / 5.4)) - s;
            const double ulp = std::nextafter((double)(s > 0 ? s : 1), DBL_MAX) - (double)(s > 0 ? s : 1);
            if (excess > 0.0L && excess <= (long double)ulp) {
                ++rounded;
                return;
            }
        }
        if (!bad++) first_bad = nA;
    };
    auto around = [&](double v) {
        probe(std::nextafter(v, 0.0));
        probe(v);
        probe(std::nextafter(v, DBL_MAX));
    };
    probe(0.0);
    probe(std::numeric_limits<double>::denorm_min());
    probe(1.0e-310);
    probe(DBL_MIN);
    probe(1.0e-300);
    const double ends[5] = {0.015, 0.25, 0.95, 2.1, 5.4};
    for (double e : ends) around(e);
    for (int s = 1; s <= 60; ++s) {
        probe(std::ldexp(5.4, s));
        probe(std::nextafter(std::ldexp(5.4, s), DBL_MAX));
    }
    probe(1.0e300);
    probe(1.7e308);
    probe(DBL_MAX);
    const int sweep = 1000000;
    const double l0 = std::log(1.0e-320), l1 = std::log(DBL_MAX);
    for (int i = 0; i <= sweep; ++i) probe(std::fmin(std::exp(l0 + (l1 - l0) * i / sweep), DBL_MAX));
    int s_max = -1, s_inf = -1, s_nan = -1;
    const int m_max = pade_degree(DBL_MAX, s_max);
    const int m_inf = pade_degree(std::numeric_limits<double>::infinity(), s_inf);
    const int m_nan = pade_degree(std::numeric_limits<double>::quiet_NaN(), s_nan);
    printf("checked %ld\nmismatches %ld\nlog2_rounded %ld\nfirst_mismatch %a\nlargest_s %d\n", checked, bad, rounded,
           first_bad, smax);
    printf("m_dbl_max %d\ns_dbl_max %d\nm_inf %d\ns_inf %d\nm_nan %d\ns_nan %d\n", m_max, s_max, m_inf, s_inf, m_nan,
           s_nan);
    for (int i = 1; i < argc; ++i) {
        int s = -1;
        const int m = pade_degree(std::strtod(argv[i], nullptr), s);
        printf("degree %s %d %d\n", argv[i], m, s);
    }
    return 0;
}
