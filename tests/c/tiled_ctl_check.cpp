// Host check of the tiled engine's control word (robustgrape_amd/csrc/grape_tiled_ctl.hpp make_ctl, taylor_top,
// julia_m_index: the lines k_tctl runs on the device) against a plain restatement: s is the smallest count >= 0
// with nA / 2^s <= 0.95, found by counting up in x87 long double (64-bit mantissa, 15-bit exponent: the division
// by a power of two is exact there for every double, denormals included), top the band of the scaled norm.
// Inputs: 0, denormals, 1e-300; the four band ends and their neighbouring doubles; 0.95 2^s and its upper
// neighbour for s = 1 .. 60; 1e300 and DBL_MAX; a log-spaced sweep of a million norms over the whole range of
// the format; +inf and NaN, which must return (s = 0).  Prints the counts, then julia_m_index of every norm given
// on the command line (hexadecimal floats), for the caller to compare with the oracle's degree choice.
#include "grape_tiled_ctl.hpp"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

static int ref_ctl(double nA) {
    int s = 0;
    const long double b0 = 0.069, b1 = 0.335, b2 = 0.826, b3 = 0.95;  // the rule's doubles, widened
    while (s < 1200 && scalbnl((long double)nA, -s) > b3) ++s;
    const long double v = scalbnl((long double)nA, -s);
    const int top = v <= b0 ? 0 : v <= b1 ? 1 : v <= b2 ? 2 : 3;
    return top | (s << 2);
}

int main(int argc, char **argv) {
    using grape_tiled::make_ctl;
    long checked = 0, bad = 0;
    int smax = 0;
    double first_bad = 0.0;
    auto probe = [&](double nA) {
        const int got = make_ctl(nA), want = ref_ctl(nA);
        ++checked;
        if ((got >> 2) > smax) smax = got >> 2;
        if (got != want && !bad++) first_bad = nA;
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
    const double ends[4] = {0.069, 0.335, 0.826, 0.95};
    for (double e : ends) around(e);
    for (int s = 1; s <= 60; ++s) {
        probe(std::ldexp(0.95, s));
        probe(std::nextafter(std::ldexp(0.95, s), DBL_MAX));
        for (int b = 0; b < 3; ++b) around(std::ldexp(ends[b], s));  // a band end after s squarings' scaling
    }
    probe(1.0e300);
    probe(1.7e308);
    probe(DBL_MAX);
    const int sweep = 1000000;
    const double l0 = std::log(1.0e-320), l1 = std::log(DBL_MAX);
    for (int i = 0; i <= sweep; ++i) probe(std::fmin(std::exp(l0 + (l1 - l0) * i / sweep), DBL_MAX));
    const int cinf = make_ctl(std::numeric_limits<double>::infinity());
    const int cnan = make_ctl(std::numeric_limits<double>::quiet_NaN());
    printf("checked %ld\nmismatches %ld\nfirst_mismatch %a\nlargest_s %d\ns_dbl_max %d\ns_inf %d\ns_nan %d\n", checked, bad,
           first_bad, smax, make_ctl(DBL_MAX) >> 2, cinf >> 2, cnan >> 2);
    for (int i = 1; i < argc; ++i)
        printf("m_index %s %d\n", argv[i], grape_tiled::julia_m_index(std::strtod(argv[i], nullptr)));
    return 0;
}
