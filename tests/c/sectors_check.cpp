// Prints the sector layout of grape_plan_setup.hpp find_sectors for a problem read from the file argv[1]:
//   d n_ops n_h0 nerr options          (options: GRAPE_OPT_* of grape_desc.reserved[1])
//   op ...                             (n_h0 operator indices: H0's terms)
//   n op ...                           (one line per error source: its terms' operator indices)
//   idle_0 ... idle_{d-1}              (0 / 1: grape_descriptor.hip idle_levels, stated by the caller)
//   then per operator: nnz, and nnz lines "row col re im"
// Output: first line "ncls nfixed"; per class a line "S nsec" and a line of nsec * S slot levels (sidx, -1:
// padding); last the fixed levels.  Host code only (tests/test_sector_shapes_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "grape_plan_setup.hpp"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int d, n_ops, n_h0, nerr, options;
    if (std::fscanf(f, "%d %d %d %d %d", &d, &n_ops, &n_h0, &nerr, &options) != 5) return 3;
    if (d < 1 || d > 64 || n_ops < 1 || n_ops > 64 || n_h0 < 0 || nerr < 0) return 3;
    auto read_op = [&](int &o) { return std::fscanf(f, "%d", &o) == 1 && o >= 0 && o < n_ops; };
    std::vector<grape_term> h0(n_h0), err;
    for (grape_term &t : h0) {
        t = grape_term{};
        if (!read_op(t.op)) return 3;
    }
    std::vector<int32_t> offs{0};
    for (int e = 0; e < nerr; ++e) {
        int n;
        if (std::fscanf(f, "%d", &n) != 1 || n < 0) return 3;
        for (int k = 0; k < n; ++k) {
            grape_term t{};
            if (!read_op(t.op)) return 3;
            err.push_back(t);
        }
        offs.push_back((int32_t)err.size());
    }
    std::vector<char> idle(d, 0);
    for (int i = 0; i < d; ++i) {
        int v;
        if (std::fscanf(f, "%d", &v) != 1) return 3;
        idle[i] = v != 0;
    }
    std::vector<double> ops(2 * (size_t)n_ops * d * d, 0.0);
    for (int o = 0; o < n_ops; ++o) {
        int nnz;
        if (std::fscanf(f, "%d", &nnz) != 1 || nnz < 0) return 3;
        for (int k = 0; k < nnz; ++k) {
            int r, c;
            double re, im;
            if (std::fscanf(f, "%d %d %lf %lf", &r, &c, &re, &im) != 4 || r < 0 || r >= d || c < 0 || c >= d) return 3;
            double *v = ops.data() + 2 * ((size_t)o * d * d + r + (size_t)c * d);
            v[0] = re;
            v[1] = im;
        }
    }
    std::fclose(f);
    grape_desc desc{};
    desc.ndim = d;
    desc.n_ops = n_ops;
    desc.nerr = nerr;
    desc.ops = ops.data();
    desc.n_h0_terms = n_h0;
    desc.h0_terms = h0.data();
    desc.err_term_offsets = nerr > 0 ? offs.data() : nullptr;
    desc.err_terms = err.data();
    desc.reserved[1] = options;
    const grape_setup::SectorSetup ss = grape_setup::find_sectors(&desc, false, &idle);
    std::printf("%zu %zu\n", ss.cls.size(), ss.fixed.size());
    for (const grape_setup::SectorClass &c : ss.cls) {
        std::printf("%d %d\n", c.S, c.nsec);
        for (int v : c.sidx) std::printf("%d ", v);
        std::printf("\n");
    }
    for (int v : ss.fixed) std::printf("%d ", v);
    std::printf("\n");
    return 0;
}
