// Prints the propagator-variant list of grape_plan_setup.hpp build_variants for
//   variants_check np nxa ne with_grad_variants      (eps = 1e-3, eps2 = 1e-2)
// first line: size off_dx off_dxa off_dx2 off_err err_stride; then one line per variant:
// var index delta err errval.  Host code only (tests/test_variants_cpu.py).
#include <cstdio>
#include <cstdlib>

#include "grape_plan_setup.hpp"

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const grape_setup::Variants V =
        grape_setup::build_variants(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), 1e-3, 1e-2, atoi(argv[4]) != 0);
    std::printf("%zu %d %d %d %d %d\n", V.vs.size(), V.off_dx, V.off_dxa, V.off_dx2, V.off_err, V.err_stride);
    for (const grape::VSpec &v : V.vs)
        std::printf("%d %d %.17g %d %.17g\n", v.pert.var, v.pert.index, v.pert.delta, v.err, v.errval);
    return 0;
}
