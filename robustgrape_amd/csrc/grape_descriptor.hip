// grape_descriptor.hip -- the pure host logic of plan creation: everything decided from the descriptor
// alone, before (and without) a device.  Validation, the factor split, the Hermiticity checks, the projector
// setup, idle levels, phase covariance (find_gauge), the symmetry-adapted view, and the route.
// No kernel, no launch and no HIP call: the types come from grape.h, grape_types.hpp, grape_plan_setup.hpp
// and grape_symmetry.hpp (grape_descriptor.hpp).  The library's compiler builds it like every unit; it is also
// plain C++17, which a host compiler builds without any HIP header (tests/c/descriptor_check.cpp links it).
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <string>
#include <vector>

#include "grape_descriptor.hpp"

namespace grape_eng {

static int validate_terms(const grape_term *t, int n, int n_ops, int np, int na, bool target, const char *what) {
    int nfac = 0;  // factor terms on the current operator term
    for (int k = 0; k < n; ++k) {
        const bool factor = t[k].op == GRAPE_OP_FACTOR;
        if (factor) {  // product coefficients: a real scalar on the closest preceding operator term of this list
            if (target) return fail(GRAPE_ERR_INVALID, std::string(what) + ": factor terms are not allowed in target terms");
            if (k == 0)
                return fail(GRAPE_ERR_INVALID, std::string(what) + ": a factor term must follow an operator term of its list");
            if (++nfac > GRAPE_MAX_FACTORS)
                return fail(GRAPE_ERR_INVALID, std::string(what) + ": more than GRAPE_MAX_FACTORS factor terms on one operator term");
            if (t[k].func < GRAPE_FN_ONE || t[k].func > GRAPE_FN_SIN)
                return fail(GRAPE_ERR_INVALID, std::string(what) + ": a factor term's func must be ONE, LINEAR, COS or SIN");
            if (t[k].scale_im != 0.0)
                return fail(GRAPE_ERR_INVALID, std::string(what) + ": a factor term's scale must be real (scale_im = 0)");
        } else {
            nfac = 0;
        }
        if (!factor && (t[k].op < 0 || t[k].op >= n_ops)) return fail(GRAPE_ERR_INVALID, std::string(what) + ": op out of range");
        if (t[k].var < 0 || t[k].var > 3) return fail(GRAPE_ERR_INVALID, std::string(what) + ": bad var");
        if (t[k].func < 0 || t[k].func > 4) return fail(GRAPE_ERR_INVALID, std::string(what) + ": bad func");
        if (t[k].var == 1 && (t[k].index < 0 || t[k].index >= np))
            return fail(GRAPE_ERR_INVALID, std::string(what) + ": control index out of range");
        if (t[k].var == 2 && (t[k].index < 0 || t[k].index >= na))
            return fail(GRAPE_ERR_INVALID, std::string(what) + ": x_add index out of range");
        if (target && (t[k].var == 1 || t[k].var == 3))
            return fail(GRAPE_ERR_INVALID, std::string(what) + ": target terms may only use x_add");
        if (!target && t[k].func == 4)
            return fail(GRAPE_ERR_INVALID, std::string(what) + ": cis coefficients only in target terms");
    }
    return GRAPE_OK;
}

static void split_list(const grape_term *t, int n, std::vector<grape_term> &ops, std::vector<grape_term> &fac,
                       FactorSplit &fs) {
    int slot = 0;
    for (int k = 0; k < n; ++k) {
        if (t[k].op != GRAPE_OP_FACTOR) {
            ops.push_back(t[k]);
            grape_term empty{};  // op = 0: an empty slot
            fac.insert(fac.end(), (size_t)GRAPE_MAX_FACTORS, empty);
            slot = 0;
        } else if (!ops.empty() && slot < GRAPE_MAX_FACTORS) {
            grape_term f = t[k];
            f.op = 1;
            fac[fac.size() - (size_t)GRAPE_MAX_FACTORS + (size_t)slot++] = f;
            fs.any = true;
            fs.reads_xadd = fs.reads_xadd || f.var == GRAPE_VAR_XADD;
            fs.reads_tstep = fs.reads_tstep || f.var == GRAPE_VAR_TSTEP;
        }
    }
}
void split_factors(const grape_desc *desc, FactorSplit &fs) {
    fs.plain = *desc;
    if ((desc->reserved[0] & GRAPE_DESC_HOST_TABLES) || !desc->h0_terms) return;
    split_list(desc->h0_terms, desc->n_h0_terms, fs.h0, fs.fac_h0, fs);
    if (desc->nerr > 0 && desc->err_term_offsets && desc->err_terms) {
        fs.err_off.push_back(0);
        for (int e = 0; e < desc->nerr; ++e) {
            const int a = desc->err_term_offsets[e], b = desc->err_term_offsets[e + 1];
            split_list(desc->err_terms + a, b - a, fs.err, fs.fac_err, fs);
            fs.err_off.push_back((int32_t)fs.err.size());
        }
    }
    if (!fs.any) return;  // the caller's descriptor as it is
    fs.plain.h0_terms = fs.h0.data();
    fs.plain.n_h0_terms = (int32_t)fs.h0.size();
    if (!fs.err_off.empty()) {
        fs.plain.err_terms = fs.err.data();
        fs.plain.err_term_offsets = fs.err_off.data();
    }
    // the stored pipeline only: no lane matrices, chains, chunk walks (so no gauge search, pair, merged or
    // wide passes) and no one-workgroup kernel -- those build generators from the plain term lists
    fs.plain.reserved[1] |= GRAPE_OPT_NO_LANE | GRAPE_OPT_NO_CHAIN | GRAPE_OPT_NO_WALK | GRAPE_OPT_NO_GAUGE |
                            GRAPE_OPT_NO_PAIR | GRAPE_OPT_NO_MERGE | GRAPE_OPT_NO_RANK1 | GRAPE_OPT_NO_WIDE |
                            GRAPE_OPT_NO_EVAL1 | GRAPE_OPT_NO_TWIN;
}

// The fused engines take C_k^-1 = C_k^dagger for the chain C_k of the NOMINAL propagators
// exp(-i dt H0) and skip balancing (a permutation only for Hermitian H): both need a
// Hermitian H0.  A term c(x) * OP keeps H0 Hermitian for every x when its function is
// real-valued and scale * OP is Hermitian; anything else (e.g. a -i Gamma/2 decay term in
// H0) selects the general-H0 path (LU inverse of the chain, grape_unitary.hip) on the small
// engine and is refused by the dense one.  Error generators need no such property:
// their propagators only enter through differences dE (UnitaryCalculations.jl:68-83) that
// the nominal chain transports, so a non-Hermitian Herror (a decay-rate error) is served.
// 0: every term keeps H Hermitian; 1: a complex-valued coefficient; 2: scale * operator not Hermitian
static int hermitian_terms(const grape_desc *desc, const grape_term *t, int n) {
    const int D = desc->ndim;
    for (int k = 0; k < n; ++k) {
        if (t[k].func == GRAPE_FN_CIS) return 1;
        const double *op = desc->ops + 2 * (size_t)t[k].op * D * D;
        const double sr = t[k].scale_re, si = t[k].scale_im;
        double mx = 0.0, dev = 0.0;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                const double *a = op + 2 * ((size_t)i + (size_t)j * D), *b = op + 2 * ((size_t)j + (size_t)i * D);
                // (s a)_ij - conj((s a)_ji)
                const double re = (sr * a[0] - si * a[1]) - (sr * b[0] - si * b[1]);
                const double im = (sr * a[1] + si * a[0]) + (sr * b[1] + si * b[0]);
                mx = std::max(mx, std::hypot(sr * a[0] - si * a[1], sr * a[1] + si * a[0]));
                dev = std::max(dev, std::hypot(re, im));
            }
        if (dev > 1e-12 * std::max(mx, 1e-300)) return 2;
    }
    return 0;
}
// The SUM of a term list Hermitian for every argument (round 6): terms with complex coefficients (each
// scale * operator non-Hermitian, e.g. e^{i a} U + e^{-i a} U^dag) whose sum is Hermitian, as the reference
// accepts any closure with a Hermitian value (UnitaryCalculations.jl:45-47).  Checked at seven probe
// arguments (controls, x_add and the step index drawn from a fixed generator): the coefficients are
// analytic in their argument, so a sum Hermitian at generic points is Hermitian everywhere.
static std::complex<double> term_value(const grape_term &t, const double *x, const double *xa, int nt1) {
    double v = 1.0;
    if (t.var == 1) v = x[t.index];
    else if (t.var == 2) v = xa[t.index];
    else if (t.var == 3) v = (double)nt1;
    const double arg = t.a * v + t.b;
    std::complex<double> f(1.0, 0.0);
    if (t.func == 1) f = arg;
    else if (t.func == 2) f = std::cos(arg);
    else if (t.func == 3) f = std::sin(arg);
    else if (t.func == 4) f = std::complex<double>(std::cos(arg), std::sin(arg));
    return std::complex<double>(t.scale_re, t.scale_im) * f;
}
static bool hermitian_sum(const grape_desc *desc, const grape_term *t, int n) {
    const int D = desc->ndim;
    uint64_t st = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() {  // splitmix64 -> [-3, 3)
        st += 0x9e3779b97f4a7c15ull;
        uint64_t z = st;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        return 6.0 * ((double)(z >> 11) * (1.0 / 9007199254740992.0)) - 3.0;
    };
    std::vector<double> x(std::max(1, desc->nparam)), xa(std::max(1, desc->nadd));
    std::vector<std::complex<double>> H((size_t)D * D);
    for (int probe = 0; probe < 7; ++probe) {
        for (double &v : x) v = rnd();
        for (double &v : xa) v = rnd();
        const int nt1 = 1 + (int)((unsigned)(probe * 7919) % (unsigned)std::max(1, desc->ntimes));
        std::fill(H.begin(), H.end(), std::complex<double>(0.0, 0.0));
        for (int k = 0; k < n; ++k) {
            const std::complex<double> c = term_value(t[k], x.data(), xa.data(), nt1);
            const double *op = desc->ops + 2 * (size_t)t[k].op * D * D;
            for (size_t e = 0; e < (size_t)D * D; ++e) H[e] += c * std::complex<double>(op[2 * e], op[2 * e + 1]);
        }
        double mx = 0.0, dev = 0.0;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                mx = std::max(mx, std::abs(H[i + (size_t)j * D]));
                dev = std::max(dev, std::abs(H[i + (size_t)j * D] - std::conj(H[j + (size_t)i * D])));
            }
        if (dev > 1e-12 * std::max(mx, 1e-300)) return false;
    }
    return true;
}
int check_hermitian_terms(const grape_desc *desc, const grape_term *t, int n, const char *what) {
    const int h = hermitian_terms(desc, t, n);
    if (h && desc->ndim > GRAPE_MAX_SMALL_DIM && hermitian_sum(desc, t, n)) return GRAPE_OK;  // dense: the sum
    if (h == 1) return fail(GRAPE_ERR_UNSUPPORTED, std::string(what) + ": complex-valued coefficient (H must be Hermitian)");
    if (h == 2)
        return fail(GRAPE_ERR_UNSUPPORTED,
                    std::string(what) + ": scale * operator is not Hermitian (non-unitary propagators are not supported)");
    return GRAPE_OK;
}

// P0 and its pattern P = P0 .!= 0 as column-major interleaved matrices
static void projector_matrices(const grape_desc *desc, std::vector<double> &P0, std::vector<double> &Pp) {
    const int D = desc->ndim;
    P0.assign(2 * (size_t)D * D, 0.0);
    Pp.assign(P0.size(), 0.0);
    for (int j = 0; j < D; ++j)
        for (int i = 0; i < D; ++i) {
            const size_t t = 2 * (i + (size_t)j * D);
            if (desc->projector) {
                P0[t] = desc->projector[t];
                P0[t + 1] = desc->projector[t + 1];
            } else if (i == j) {
                P0[t] = desc->projector_diag[i];
            }
            Pp[t] = (P0[t] != 0.0 || P0[t + 1] != 0.0) ? 1.0 : 0.0;
        }
}
// ... the setup from them (the caller's, or rotated ones: the symmetry-adapted sectors, whose pattern
// is the rotated P, not the pattern of the rotated P0)
static ProjectorSetup projector_from(const double *P0, const double *Pp, int D) {
    ProjectorSetup ps;
    ps.W.assign(D, 0.0);
    ps.P0.resize((size_t)D * D);
    std::vector<cd> B((size_t)D * D);
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {  // row-major tiles
            const size_t t = 2 * (i + (size_t)j * D);
            ps.P0[(size_t)i * D + j] = cd{P0[t], P0[t + 1]};
            B[(size_t)i * D + j] = cd{Pp[t], Pp[t + 1]};
            if (i == j) {
                ps.trP += P0[t];
                ps.W[i] = P0[t];
                // the diagonal specialisation needs P = diag(P0 != 0) exactly
                const double pat = P0[t] != 0.0 ? 1.0 : 0.0;
                if (P0[t + 1] != 0.0 || Pp[t + 1] != 0.0 || std::fabs(Pp[t] - pat) > 1e-14) ps.general = true;
            } else if (P0[t] != 0.0 || P0[t + 1] != 0.0 || Pp[t] != 0.0 || Pp[t + 1] != 0.0) {
                ps.general = true;
            }
        }
    if (ps.general) ps.set_general(D, B);
    return ps;
}
ProjectorSetup setup_projector(const grape_desc *desc) {
    std::vector<double> P0, Pp;
    projector_matrices(desc, P0, Pp);
    return projector_from(P0.data(), Pp.data(), desc->ndim);
}

// Levels that cannot reach F or a derivative of it when no operator couples them to another level (find_sectors):
// diagonal projector (in the sector path's basis) without weight on the level, and every target operator free of
// entries beside the diagonal in the level's row and column.
std::vector<char> idle_levels(const grape_desc *desc, const grape_desc &sdesc, const ProjectorSetup &sps) {
    const int D = desc->ndim;
    std::vector<char> idle(D, 0);
    if (sps.general || !desc->target_terms) return idle;
    for (int g = 0; g < D; ++g) idle[g] = sps.W[g] == 0.0;
    for (int k = 0; k < desc->n_target_terms; ++k) {
        const double *op = sdesc.ops + 2 * (size_t)desc->target_terms[k].op * D * D;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j)
                if (i != j && (op[2 * (i + (size_t)j * D)] != 0.0 || op[2 * (i + (size_t)j * D) + 1] != 0.0))
                    idle[i] = idle[j] = 0;
    }
    return idle;
}

// Phase covariance of a sector class (grape_walk.hpp GAUGE): does every sector block obey
// H_w(x) = D(a x) H_w(0) D(a x)^dag, D(t) = diag(e^{i t N_j}), for the one control x?  Needs np = 1,
// H0 and every error source's terms free of x_add and of the step index (error sources are accepted:
// their terms must be covariant with the same charges, k_walk_img_gauge), and every term that reads x
// a cos / sin / cis of a x + b with one common a.  The charges come from the ratios of the blocks'
// entries at a small x to their values at x = 0 (N_j - N_k = n_jk, integer), propagated over each
// sector's coupling graph; the identity is then checked entry by entry at seven x values (a
// rotated basis -- the symmetry-adapted sectors -- is covered: the blocks are the rotated ones).
// On success N holds [nsec][S] charges >= 0 (0 on padding slots) and a the common factor.
bool find_gauge(const grape_desc *desc, const grape_desc &sdesc, const SectorClass &sc, double &a,
                       std::vector<int> &N) {
    constexpr int kMaxCharge = 8;
    const int D = desc->ndim, S = sc.S, NE = desc->nerr;
    const size_t T = (size_t)D * D;
    if (desc->nparam != 1) return false;
    // the term lists: H0's, then every error source's (UnitaryCalculations.jl:67-97 adds
    // errval * Herror_e to H0: both must be covariant with the same charges)
    std::vector<std::pair<const grape_term *, int>> lists{{desc->h0_terms, desc->n_h0_terms}};
    for (int e = 0; e < NE; ++e)
        lists.push_back({desc->err_terms + desc->err_term_offsets[e],
                         desc->err_term_offsets[e + 1] - desc->err_term_offsets[e]});
    bool have_a = false;
    a = 1.0;
    for (const auto &l : lists)
        for (int t = 0; t < l.second; ++t) {
            const grape_term &tm = l.first[t];
            if (tm.var == 2 || tm.var == 3) return false;  // x_add or the step index
            if (tm.var != 1) continue;
            if (tm.func != 2 && tm.func != 3 && tm.func != 4) return false;  // x must enter as a phase
            if (!(tm.a != 0.0) || (have_a && tm.a != a)) return false;
            a = tm.a;
            have_a = true;
        }
    auto block = [&](int w, int li, double x, std::vector<std::complex<double>> &H) {
        H.assign((size_t)S * S, 0.0);
        for (int t = 0; t < lists[li].second; ++t) {
            const grape_term &tm = lists[li].first[t];
            const std::complex<double> c = term_value(tm, &x, nullptr, 0);  // (no x_add, no step index: checked above)
            for (int r = 0; r < S; ++r)
                for (int q = 0; q < S; ++q) {
                    const int gi = sc.sidx[(size_t)w * S + r], gj = sc.sidx[(size_t)w * S + q];
                    if (gi < 0 || gj < 0) continue;
                    const double *v = sdesc.ops + 2 * ((size_t)tm.op * T + gi + (size_t)gj * D);
                    H[(size_t)r * S + q] += c * std::complex<double>(v[0], v[1]);
                }
        }
    };
    N.assign((size_t)sc.nsec * S, 0);
    const double xs = 0.01 / std::fabs(a);
    const double probe[7] = {0.37, -1.3, 2.9, 7.77, -31.4, 0.001, 123.456};
    const int NL = (int)lists.size();
    std::vector<std::vector<std::complex<double>>> H0(NL), Hs(NL);
    std::vector<std::complex<double>> Hx;
    std::vector<double> tol(NL);
    for (int w = 0; w < sc.nsec; ++w) {
        // charge differences n_rq = N_r - N_q from every block's entries (H0's and the errors')
        std::vector<int> n((size_t)S * S, 0);
        std::vector<char> cpl((size_t)S * S, 0);
        for (int li = 0; li < NL; ++li) {
            block(w, li, 0.0, H0[li]);
            block(w, li, xs, Hs[li]);
            double hmax = 0.0;
            for (const auto &h : H0[li]) hmax = std::max(hmax, std::abs(h));
            for (const auto &h : Hs[li]) hmax = std::max(hmax, std::abs(h));
            tol[li] = 1e-13 * std::max(hmax, 1e-300);
            for (int r = 0; r < S; ++r)
                for (int q = 0; q < S; ++q) {
                    const std::complex<double> h0 = H0[li][(size_t)r * S + q], h1 = Hs[li][(size_t)r * S + q];
                    if (std::abs(h0) <= tol[li]) {
                        if (std::abs(h1) > tol[li]) return false;  // vanishes at x = 0 only: not a phase
                        continue;
                    }
                    const double m = std::arg(h1 / h0) / (a * xs);
                    const int nn = (int)std::lround(m);
                    if (std::fabs(m - nn) > 1e-6 || std::abs(nn) > kMaxCharge || (r == q && nn != 0)) return false;
                    if (cpl[(size_t)r * S + q] && n[(size_t)r * S + q] != nn) return false;
                    cpl[(size_t)r * S + q] = 1;
                    n[(size_t)r * S + q] = nn;
                }
        }
        std::vector<int> Nw(S, 0);  // charges by breadth-first search over the couplings
        std::vector<char> seen(S, 0);
        for (int s0 = 0; s0 < S; ++s0) {
            if (seen[s0]) continue;
            seen[s0] = 1;
            std::vector<int> stack{s0};
            while (!stack.empty()) {
                const int r = stack.back();
                stack.pop_back();
                for (int q = 0; q < S; ++q) {
                    if (!cpl[(size_t)r * S + q]) continue;
                    const int want = Nw[r] - n[(size_t)r * S + q];  // n_rq = N_r - N_q
                    if (!seen[q]) {
                        seen[q] = 1;
                        Nw[q] = want;
                        stack.push_back(q);
                    } else if (Nw[q] != want) {
                        return false;
                    }
                }
            }
        }
        const int lo = *std::min_element(Nw.begin(), Nw.end());
        for (int r = 0; r < S; ++r) {
            Nw[r] -= lo;
            if (Nw[r] > kMaxCharge) return false;
            N[(size_t)w * S + r] = Nw[r];
        }
        for (int li = 0; li < NL; ++li)
            for (double x : probe) {  // the identity itself, entry by entry, every block
                block(w, li, x, Hx);
                double hm = tol[li] * 1e13;
                for (const auto &h : Hx) hm = std::max(hm, std::abs(h));
                for (int r = 0; r < S; ++r)
                    for (int q = 0; q < S; ++q) {
                        const std::complex<double> ph = std::polar(1.0, a * x * (Nw[r] - Nw[q]));
                        if (std::abs(Hx[(size_t)r * S + q] - ph * H0[li][(size_t)r * S + q]) > 1e-12 * std::max(hm, 1e-300))
                            return false;
                    }
            }
    }
    return true;
}

static std::vector<const double *> used_operators(const grape_desc *desc) {
    std::vector<const double *> u;
    const int D = desc->ndim;
    for (int t = 0; t < desc->n_h0_terms; ++t) u.push_back(desc->ops + 2 * (size_t)desc->h0_terms[t].op * D * D);
    const int ne = desc->nerr > 0 ? desc->err_term_offsets[desc->nerr] : 0;
    for (int t = 0; t < ne; ++t) u.push_back(desc->ops + 2 * (size_t)desc->err_terms[t].op * D * D);
    return u;
}
static void snap_residue(double *m, int D, double rel) {  // m: D x D interleaved
    double big = 0.0;
    for (int t = 0; t < 2 * D * D; ++t) big = std::max(big, std::fabs(m[t]));
    for (int t = 0; t < 2 * D * D; ++t)
        if (std::fabs(m[t]) <= rel * big) m[t] = 0.0;
}
SymSetup symmetry_setup(const grape_desc *desc) {
    SymSetup sy;
    const int D = desc->ndim;
    if (D > GRAPE_MAX_SMALL_DIM || (desc->reserved[1] & (GRAPE_OPT_NO_SYMMETRY | GRAPE_OPT_NO_SECTORS))) return sy;
    sy.split = grape_sym::symmetry_split(D, used_operators(desc));
    if (!sy.split.rotated) return sy;
    const size_t T2 = 2 * (size_t)D * D;
    sy.ops.assign((size_t)desc->n_ops * T2, 0.0);
    std::vector<char> used(desc->n_ops, 0);
    for (int t = 0; t < desc->n_h0_terms; ++t) used[desc->h0_terms[t].op] = 1;
    const int ne = desc->nerr > 0 ? desc->err_term_offsets[desc->nerr] : 0;
    for (int t = 0; t < ne; ++t) used[desc->err_terms[t].op] = 1;
    for (int o = 0; o < desc->n_ops; ++o) {
        double *r = sy.ops.data() + (size_t)o * T2;
        grape_sym::rotate(sy.split, desc->ops + (size_t)o * T2, r);
        if (used[o])  // off the invariant blocks: zero by construction (checked in symmetry_split)
            for (int j = 0; j < D; ++j)
                for (int i = 0; i < D; ++i)
                    if (sy.split.block[i] != sy.split.block[j]) r[2 * (i + (size_t)j * D)] = r[2 * (i + (size_t)j * D) + 1] = 0.0;
        snap_residue(r, D, 1e-15);
    }
    // the projector P0 and its pattern P in the rotated basis
    std::vector<double> P0, Pp, P0r(T2), Ppr(T2);
    projector_matrices(desc, P0, Pp);
    grape_sym::rotate(sy.split, P0.data(), P0r.data());
    grape_sym::rotate(sy.split, Pp.data(), Ppr.data());
    snap_residue(P0r.data(), D, 1e-15);
    snap_residue(Ppr.data(), D, 1e-15);
    sy.ps = projector_from(P0r.data(), Ppr.data(), D);
    // worth it only when the rotated sectors are cheaper than the permutation ones
    const grape_desc rv = sy.view(desc);
    const SectorSetup rot = find_sectors(&rv, false), perm = find_sectors(desc, false);
    if (rot.cls.empty()) return sy;
    long crot = 0, cperm = 0;
    for (const SectorClass &c : rot.cls) crot += sector_cost(c);
    for (const SectorClass &c : perm.cls) cperm += sector_cost(c);
    if (perm.cls.empty()) cperm = (long)D * D * D;
    sy.on = crot < cperm;
    return sy;
}

// Everything checkable without a device, in this order (a machine without one sees these codes
// before GRAPE_ERR_NO_DEVICE).
int validate_desc(const grape_desc *desc, int *n_err_terms) {
    const int D = desc->ndim;
    const bool tables = (desc->reserved[0] & GRAPE_DESC_HOST_TABLES) != 0;
    if (D < 2 || desc->ntimes < 1 || desc->nparam < 1 || desc->nadd < 0 || desc->nerr < 0 ||
        (!tables && desc->n_ops < 1))
        return fail(GRAPE_ERR_INVALID, "bad dimensions in descriptor");
    if (D > GRAPE_MAX_TILED_DIM) return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_TILED_DIM");
    if (D > GRAPE_MAX_DENSE_DIM) {  // the tiled engine: what it does not serve is refused here, before any device work
        if (tables)
            return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: closures (host tables) are served up to "
                                               "GRAPE_MAX_DENSE_DIM levels");
        const bool tiled_err = (desc->reserved[1] & GRAPE_OPT_TILED_ERR) != 0;
        if (desc->nerr > 0 && !tiled_err)
            return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: error sources are served up to "
                                               "GRAPE_MAX_DENSE_DIM levels");
        if (desc->reserved[1] & GRAPE_OPT_GENERAL_H0)
            return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: GRAPE_OPT_GENERAL_H0 is served up to "
                                               "GRAPE_MAX_DENSE_DIM levels (the tiled engine needs a Hermitian H0)");
        if (desc->n_h0_terms > grape_tiled::kMaxTerms || desc->n_target_terms > grape_tiled::kMaxTerms)
            return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: more than 256 H0 or target terms");
    }
    if (tables) {  // above GRAPE_MAX_SMALL_DIM: the general path with the dense exponential of the tables
        if (!desc->projector_diag && !desc->projector) return fail(GRAPE_ERR_INVALID, "missing projector");
    } else {
        if (desc->nerr > 0 && !desc->err_term_offsets) return fail(GRAPE_ERR_INVALID, "missing err_term_offsets");
        if (!desc->ops || !desc->h0_terms || desc->n_h0_terms < 1 || (!desc->projector_diag && !desc->projector) ||
            !desc->target_terms || desc->n_target_terms < 1)
            return fail(GRAPE_ERR_INVALID, "missing operator basis / terms / projector");
    }
    if (!(desc->t0 > 0) || !(desc->eps > 0)) return fail(GRAPE_ERR_INVALID, "t0 and eps must be positive");
    int rc;
    if (!tables && (rc = validate_terms(desc->h0_terms, desc->n_h0_terms, desc->n_ops, desc->nparam, desc->nadd, false, "H0")))
        return rc;
    if (!tables && (rc = validate_terms(desc->target_terms, desc->n_target_terms, desc->n_ops, desc->nparam, desc->nadd, true,
                             "target")))
        return rc;
    *n_err_terms = 0;
    if (desc->nerr > 0 && !tables) {
        for (int e = 0; e < desc->nerr; ++e)
            if (desc->err_term_offsets[e + 1] <= desc->err_term_offsets[e])
                return fail(GRAPE_ERR_INVALID, "each error source needs at least one term");
        if (desc->err_term_offsets[0] != 0) return fail(GRAPE_ERR_INVALID, "err_term_offsets[0] must be 0");
        *n_err_terms = desc->err_term_offsets[desc->nerr];
        for (int e = 0; e < desc->nerr; ++e)  // per source: a factor term never starts a source's range
            if ((rc = validate_terms(desc->err_terms + desc->err_term_offsets[e],
                                     desc->err_term_offsets[e + 1] - desc->err_term_offsets[e], desc->n_ops, desc->nparam,
                                     desc->nadd, false, "error source")))
                return rc;
    }
    if (!tables && D > GRAPE_MAX_SMALL_DIM) {  // product coefficients: the small engine's stored pipeline only
        bool any = false;
        for (int k = 0; k < desc->n_h0_terms; ++k) any = any || desc->h0_terms[k].op == GRAPE_OP_FACTOR;
        for (int k = 0; k < *n_err_terms; ++k) any = any || desc->err_terms[k].op == GRAPE_OP_FACTOR;
        if (any)
            return fail(GRAPE_ERR_UNSUPPORTED, "product coefficients (factor terms) are served up to GRAPE_MAX_SMALL_DIM "
                                               "levels; the dense and tiled engines do not take them");
    }
    return GRAPE_OK;
}

int choose_route(const grape_desc *desc, int n_err_terms, Route &rt) {
    const int D = desc->ndim;
    rt.tables = (desc->reserved[0] & GRAPE_DESC_HOST_TABLES) != 0;
    rt.general_h0 = (desc->reserved[1] & GRAPE_OPT_GENERAL_H0) != 0;
    if (!rt.tables && !rt.general_h0)
        if (int rc = check_hermitian_terms(desc, desc->h0_terms, desc->n_h0_terms, "H0")) {
            if (rc != GRAPE_ERR_UNSUPPORTED || D > GRAPE_MAX_SMALL_DIM) return rc;
            rt.general_h0 = true;  // non-Hermitian H0: the general path serves it
        }
    // 12 < d <= 64 with the option: the general path over the dense engine's pivoted exponential
    // (operator bases: setup_pivot_dense, after the general-path problem; host tables:
    // launch_table_variants).  Without the option nothing changes: a non-Hermitian H0 or error source
    // is refused above.
    rt.pivot = rt.general_h0 && D > GRAPE_MAX_SMALL_DIM;
    if (D > GRAPE_MAX_DENSE_DIM) {  // the tiled engine (validate_desc refused closures, the general option, and error
                                    // sources without GRAPE_OPT_TILED_ERR)
        for (int k = 0; k < desc->n_h0_terms; ++k)
            if (desc->h0_terms[k].var == GRAPE_VAR_XADD)
                return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: H0 terms that read x_add are served up "
                                                   "to GRAPE_MAX_DENSE_DIM levels");
        // error sources (GRAPE_OPT_TILED_ERR, let through by validate_desc): Hermitian, off x_add, and few enough
        // terms that a variant's coefficients -- H0's, then one source's -- are staged in LDS together
        int most = 0;
        for (int e = 0; e < desc->nerr; ++e) {
            const grape_term *t = desc->err_terms + desc->err_term_offsets[e];
            const int n = desc->err_term_offsets[e + 1] - desc->err_term_offsets[e];
            for (int k = 0; k < n; ++k)
                if (t[k].var == GRAPE_VAR_XADD)
                    return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: error terms that read x_add are "
                                                       "served up to GRAPE_MAX_DENSE_DIM levels");
            if (int rc = check_hermitian_terms(desc, t, n, "error source (tiled engine)")) return rc;
            most = std::max(most, n);
        }
        if (desc->nerr > 0 && desc->n_h0_terms + most > grape_tiled::kMaxTerms)
            return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: more than 256 terms in H0 and one error "
                                               "source together");
        if (desc->projector) {
            const size_t n = (size_t)D;
            for (size_t j = 0; j < n; ++j)
                for (size_t i = 0; i < n; ++i) {
                    const double *e = desc->projector + 2 * (i + j * n);
                    if ((i != j && (e[0] != 0.0 || e[1] != 0.0)) || (i == j && e[1] != 0.0))
                        return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: a non-diagonal projector is "
                                                           "served up to GRAPE_MAX_DENSE_DIM levels");
                }
        }
    }
    // closures above the small engine: host tables through the general path (materialised
    // derivatives), each tabulated generator exponentiated by the dense engine (grape_dense.hip
    // launch_table_variants; the host checks that the tables are Hermitian)
    if (rt.tables && D > GRAPE_MAX_SMALL_DIM) rt.general_h0 = true;
    // host tables: H0 / Herror are opaque closures that may read x_add, so every x_add call
    // site of the reference is tabulated (UnitaryCalculations.jl:57-64, 87-95)
    rt.xadd_dep = rt.tables && desc->nadd > 0;
    for (int k = 0; k < (rt.tables ? 0 : desc->n_h0_terms); ++k)
        if (desc->h0_terms[k].var == 2) rt.xadd_dep = true;
    for (int k = 0; k < n_err_terms; ++k)
        if (desc->err_terms[k].var == 2) rt.xadd_dep = true;
    // Hermitian error generators (the image walk's exponential is skew-Hermitian, grape_walk.hpp)
    rt.err_herm = rt.tables || hermitian_terms(desc, desc->err_terms, n_err_terms) == 0;
    return GRAPE_OK;
}

}  // namespace grape_eng
using namespace grape_eng;

extern "C" int grape_symmetry_basis(const grape_desc *desc, double *V, int *block) {
    if (!desc || !V || desc->ndim < 1 || desc->ndim > GRAPE_MAX_SMALL_DIM || !desc->ops || desc->n_ops < 1)
        return fail(GRAPE_ERR_INVALID, "grape_symmetry_basis: operator-basis descriptor with 1 <= ndim <= 12");
    const int D = desc->ndim;
    for (int t = 0; t < desc->n_h0_terms; ++t)
        if (desc->h0_terms[t].op != GRAPE_OP_FACTOR && (desc->h0_terms[t].op < 0 || desc->h0_terms[t].op >= desc->n_ops))
            return fail(GRAPE_ERR_INVALID, "bad op index");
    FactorSplit fs;  // factor terms carry no operator: the operator terms alone span the algebra
    split_factors(desc, fs);
    desc = &fs.plain;
    const grape_sym::Split sp = grape_sym::symmetry_split(D, used_operators(desc));
    for (size_t t = 0; t < sp.V.size(); ++t) {
        V[2 * t] = sp.V[t].real();
        V[2 * t + 1] = sp.V[t].imag();
    }
    if (block)
        for (int i = 0; i < D; ++i) block[i] = sp.block[i];
    return sp.rotated ? 1 : 0;
}
