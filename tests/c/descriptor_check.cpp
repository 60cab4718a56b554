// The descriptor logic of plan creation (grape_descriptor.hip) and the sector layout rule (grape_plan_setup.hpp
// find_sectors), linked into a host program: compiled with grape_descriptor.hip as plain C++ under
// AddressSanitizer and UBSan (tests/test_sector_shapes_cpu.py).  Reads a problem from the file argv[1]:
//   d n_ops n_h0 nerr options          (options: GRAPE_OPT_* of grape_desc.reserved[1])
//   op ...                             (n_h0 operator indices: H0's terms)
//   n op ...                           (one line per error source: its terms' operator indices)
//   n op ...                           (the target terms' operator indices)
//   ntimes nparam nadd
//   "diag" w_0 ... w_{d-1}  |  "full" and d * d pairs "re im", column-major      (the projector)
//   "ok" | "op" | "offsets"            (the descriptor as it is | H0's last term with op = n_ops | decreasing
//                                       err_term_offsets: malformed descriptors that validate_desc refuses)
//   then per operator: nnz, and nnz lines "row col re im"
// Output: "validate <rc> <message>"; when rc is GRAPE_OK: "route <rc>", the idle mask (idle_levels without the
// symmetry view: the descriptor's own operators), "ncls nfixed", per class a line "S nsec" and a line of
// nsec * S slot levels (sidx, -1: padding), last the fixed levels.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "grape_descriptor.hpp"

static std::string g_msg;
int grape_eng::fail(int code, const std::string &msg) {
    g_msg = msg;
    return code;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int d, n_ops, n_h0, nerr, options;
    if (std::fscanf(f, "%d %d %d %d %d", &d, &n_ops, &n_h0, &nerr, &options) != 5) return 3;
    if (d < 1 || d > 64 || n_ops < 1 || n_ops > 64 || n_h0 < 1 || nerr < 0) return 3;
    auto read_terms = [&](int n, std::vector<grape_term> &out) {
        for (int k = 0; k < n; ++k) {
            grape_term t{};  // a constant coefficient: var = GRAPE_VAR_ONE, func = GRAPE_FN_ONE
            t.scale_re = 1.0;
            if (std::fscanf(f, "%d", &t.op) != 1 || t.op < 0 || t.op >= n_ops) return false;
            out.push_back(t);
        }
        return true;
    };
    std::vector<grape_term> h0, err, tgt;
    if (!read_terms(n_h0, h0)) return 3;
    std::vector<int32_t> offs{0};
    for (int e = 0; e < nerr; ++e) {
        int n;
        if (std::fscanf(f, "%d", &n) != 1 || n < 0 || !read_terms(n, err)) return 3;
        offs.push_back((int32_t)err.size());
    }
    int n_tgt, ntimes, nparam, nadd;
    if (std::fscanf(f, "%d", &n_tgt) != 1 || n_tgt < 1 || !read_terms(n_tgt, tgt)) return 3;
    if (std::fscanf(f, "%d %d %d", &ntimes, &nparam, &nadd) != 3) return 3;
    char word[16];
    if (std::fscanf(f, "%15s", word) != 1) return 3;
    const bool full = std::strcmp(word, "full") == 0;
    if (!full && std::strcmp(word, "diag") != 0) return 3;
    std::vector<double> proj(full ? 2 * (size_t)d * d : (size_t)d);
    for (double &v : proj)
        if (std::fscanf(f, "%lf", &v) != 1) return 3;
    if (std::fscanf(f, "%15s", word) != 1) return 3;
    const std::string broken = word;
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
    desc.ntimes = ntimes;
    desc.nparam = nparam;
    desc.nadd = nadd;
    desc.n_ops = n_ops;
    desc.nerr = nerr;
    desc.t0 = 1.0;
    desc.eps = 1e-4;
    desc.ops = ops.data();
    desc.n_h0_terms = n_h0;
    desc.h0_terms = h0.data();
    desc.n_target_terms = n_tgt;
    desc.target_terms = tgt.data();
    desc.err_term_offsets = nerr > 0 ? offs.data() : nullptr;
    desc.err_terms = err.data();
    (full ? desc.projector : desc.projector_diag) = proj.data();
    desc.reserved[1] = options;
    if (broken == "op") {
        h0.back().op = n_ops;
    } else if (broken == "offsets") {
        if (nerr < 2 || offs[1] < 1) return 3;
        offs[2] = offs[1] - 1;
    } else if (broken != "ok") {
        return 3;
    }
    int n_err_terms = -1;
    const int rc = grape_eng::validate_desc(&desc, &n_err_terms);
    std::printf("validate %d %s\n", rc, g_msg.c_str());
    if (rc != GRAPE_OK) return 0;
    if (n_err_terms != (int)err.size()) return 4;
    grape_eng::Route rt;
    std::printf("route %d\n", grape_eng::choose_route(&desc, n_err_terms, rt));
    const grape_eng::ProjectorSetup ps = grape_eng::setup_projector(&desc);
    const std::vector<char> idle = grape_eng::idle_levels(&desc, desc, ps);
    for (char v : idle) std::printf("%d ", (int)v);
    std::printf("\n");
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
