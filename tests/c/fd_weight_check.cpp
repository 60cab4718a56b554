// Host check of the wide gradient walk's difference weights (robustgrape_amd/csrc/grape_fd_weight.hpp): the
// per-plan base plus first-order term against the per-step form (cis_m1 and the recurrence), both measured
// against e^{i m phi} - 1 in x87 long double at the exact phase phi = a h, h = fl(x + eps) - x, for m = 1, 2, 3.
// Errors are |value - exact| in units of 2^-52 |rho(m)|.  Inputs: a in {1, -2.5, 0.5}; eps = 1e-8 and one eps
// above 0.05 / |a| (the base through the library sine); x = +-0, a grid and random points of [0, 0.0063], the
// neighbourhood of +-40, the largest |x| whose step phase a x the table form accepts, random magnitudes in
// between, and x so large that x + eps rounds to x or to x plus a unit of x's last place well away from eps
// (the guard must send those to the per-step form).  Prints both worst errors, the number of inputs with h == eps
// and how many of them differ in a bit from the per-step form, and the same for the inputs the guard must refuse.
#include "grape_cis.hpp"
#include "grape_fd_weight.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

using namespace grape_fd;

static bool same_bits(Z a, Z b) { return std::memcmp(&a.re, &b.re, 8) == 0 && std::memcmp(&a.im, &b.im, 8) == 0; }

int main() {
    constexpr int kM = 3;
    const long double kUnit = 2.220446049250313e-16L;
    double worst_parent = 0, worst_new = 0;
    long n_exact = 0, exact_mismatch = 0, n_fast = 0, n_slow = 0, n_refuse = 0, refuse_wrong = 0;
    const double as[3] = {1.0, -2.5, 0.5};
    for (double a : as) {
        const double epss[2] = {1.0e-8, 0.06 / std::fabs(a)};
        for (double eps : epss) {
            Base base[kM + 1];
            for (int m = 1; m <= kM; ++m) base[m] = fd_base_h(fd_base(a * eps, m), a);
            const double thr = fd_threshold_h(a, eps, kM);
            // must_refuse: the input is one the guard has to hand to the per-step form
            auto probe = [&](double x, bool must_refuse) {
                const double xe = x + eps, h = xe - x, dh = h - eps;
                const bool fast = std::fabs(dh) <= thr;
                const Z q = cis_m1(a * h);
                const long double phi = (long double)a * (long double)h;
                for (int m = 1; m <= kM; ++m) {
                    const Z par = rho_pow(q, m), neu = fast ? fd_step(base[m], dh) : par;
                    const long double sh = sinl(0.5L * m * phi), re = -2.0L * sh * sh, im = sinl(m * phi);
                    const long double mod = hypotl(re, im);
                    if (mod > 0) {
                        worst_parent = std::fmax(worst_parent, (double)(hypotl(par.re - re, par.im - im) / (kUnit * mod)));
                        worst_new = std::fmax(worst_new, (double)(hypotl(neu.re - re, neu.im - im) / (kUnit * mod)));
                    } else if (neu.re != 0.0 || neu.im != 0.0) {
                        worst_new = INFINITY;  // (h == 0: the weights are exactly zero)
                    }
                    if (h == eps) exact_mismatch += !same_bits(par, neu);
                    if (must_refuse) refuse_wrong += fast || !same_bits(par, neu);
                }
                n_exact += h == eps;
                n_refuse += must_refuse;
                (fast ? n_fast : n_slow)++;
            };
            probe(0.0, false);
            probe(-0.0, false);
            const int grid = 200000;
            for (int i = 0; i <= grid; ++i) probe(0.0063 * i / grid, false);
            std::mt19937_64 g(7);
            std::uniform_real_distribution<double> bench(0.0, 0.0063), near40(-1.0e-3, 1.0e-3), expo(-12.0, 0.0);
            for (int i = 0; i < 200000; ++i) {
                probe(bench(g), false);
                probe(-bench(g), false);
                probe(40.0 + near40(g), false);
                probe(-40.0 + near40(g), false);
            }
            const double xmax = grape_cis::kCisTabFast / std::fabs(a);  // |a x| at the table form's bound
            for (int i = 0; i < 200000; ++i) {
                const double mag = xmax * std::pow(10.0, expo(g));
                probe(mag, false);
                probe(-mag, false);
            }
            probe(xmax, false);
            probe(-xmax, false);
            probe(std::nextafter(xmax, 0.0), false);
            // x + eps rounds to x (h = 0), or to the next double with a unit in the last place of 1.49 eps
            // (h = 1.49 eps) or 0.745 eps (h = 0.745 eps or 1.49 eps)
            const double big[3] = {eps * 0x1p56, eps * 0x1p52 * 1.49 * 1.2, eps * 0x1p52 * 0.745 * 1.2};
            for (double b : big) {
                for (int i = 0; i < 1000; ++i) {
                    const double x = b * (1.0 + 1.0e-3 * i / 1000);
                    const double h = (x + eps) - x;
                    const bool off = !(std::fabs(h - eps) <= 0.2 * eps);
                    probe(x, off);
                    probe(-x, !(std::fabs(((-x) + eps) - (-x) - eps) <= 0.2 * eps));
                }
            }
        }
    }
    printf("parent_err %.4f\nnew_err %.4f\nn_exact %ld\nexact_mismatch %ld\nn_fast %ld\nn_slow %ld\nn_refuse %ld\nrefuse_wrong %ld\n",
           worst_parent, worst_new, n_exact, exact_mismatch, n_fast, n_slow, n_refuse, refuse_wrong);
    return 0;
}
