// grape_plan_setup.hpp -- host-side pieces of plan construction (grape_plan_build.hip): the propagator
// variant list, the operator / projector tile layouts, and the sector layout rule (find_sectors).
// Plain C++: no kernel, no launch and no HIP header, so host programs compile it (tests/c).
#pragma once
#include <algorithm>
#include <vector>

#include "grape.h"
#include "grape_types.hpp"

namespace grape_setup {

using grape::cd;

// Propagator variants of one step (the closure call sites of UnitaryCalculations.jl:45-95):
//   0 nominal | dx: x_p + eps (np) | dxa: x_add_q + eps (nxa) | ne > 0: dx2: x_p + eps2, then
//   x_add_q + eps2 | per error e: err(eps), err2(eps2), mix_p (x_p + eps2, err eps2), then mix_q
//   (x_add_q + eps2, err eps2)
// nxa: na only if H0 reads x_add, otherwise exp(A(x_add + eps)) == exp(A) bit for bit and the
// reference's difference is 0 (the analysis entry points and the host-table layout keep every x_add
// site).  The eps2 variants only feed the mixed stencils: skipped when ne == 0 (dead work).
// with_grad_variants = false drops dx / dxa too (dense engine without error sources: k_dgrad
// exponentiates its variants in place).  "u" indexes the np + nxa gradient parameters, controls then
// x_add: off_dx + u, off_dx2 + u and off_err + e * err_stride + 2 + u are the variants of parameter u.
struct Variants {
    std::vector<grape::VSpec> vs;
    int off_dx, off_dxa, off_dx2, off_err, err_stride;
};
inline Variants build_variants(int np, int nxa, int ne, double eps, double eps2, bool with_grad_variants) {
    Variants V;
    auto addv = [&](int var, int idx, double delta, int err, double errval) {
        grape::VSpec v;
        v.pert.var = var;
        v.pert.index = idx;
        v.pert.delta = delta;
        v.err = err;
        v.errval = errval;
        V.vs.push_back(v);
    };
    auto params = [&](double delta, int err, double errval) {  // controls, then x_add
        for (int q = 0; q < np; ++q) addv(1, q, delta, err, errval);
        for (int q = 0; q < nxa; ++q) addv(2, q, delta, err, errval);
    };
    addv(-1, 0, 0.0, -1, 0.0);
    V.off_dx = (int)V.vs.size();
    V.off_dxa = V.off_dx + (with_grad_variants ? np : 0);
    if (with_grad_variants) params(eps, -1, 0.0);
    V.off_dx2 = (int)V.vs.size();
    if (ne > 0) params(eps2, -1, 0.0);
    V.off_err = (int)V.vs.size();
    V.err_stride = 2 + np + nxa;
    for (int e = 0; e < ne; ++e) {
        addv(-1, 0, 0.0, e, eps);
        addv(-1, 0, 0.0, e, eps2);
        params(eps2, e, eps2);
    }
    return V;
}

// Operator basis: column-major interleaved d x d matrices -> row-major cd tiles (row builds) and
// column-major ones (the exp kernels build columns; col may be null).  With sidx ([nsec][S]: the level
// in slot a of sector w, or -1 for padding) the S x S blocks of every sector, [w][o][S][S]; sidx
// null: the whole matrices (nsec = 1, S = D).
inline void to_tiles(const double *ops, int n_ops, int D, const int *sidx, int nsec, int S, cd *row, cd *col) {
    const size_t T = (size_t)D * D, TS = (size_t)S * S;
    for (int w = 0; w < nsec; ++w)
        for (int o = 0; o < n_ops; ++o)
            for (int a = 0; a < S; ++a)
                for (int c = 0; c < S; ++c) {
                    const int gi = sidx ? sidx[(size_t)w * S + a] : a, gj = sidx ? sidx[(size_t)w * S + c] : c;
                    cd v{0.0, 0.0};
                    if (gi >= 0 && gj >= 0) {
                        const double *sv = ops + 2 * ((size_t)o * T + gi + (size_t)gj * D);
                        v = cd{sv[0], sv[1]};
                    }
                    const size_t base = ((size_t)w * n_ops + o) * TS;
                    row[base + (size_t)a * S + c] = v;
                    if (col) col[base + (size_t)c * S + a] = v;
                }
}

// a diagonal projector as the heads' tiles: A = diag(w), B = diag(w != 0)
inline void diag_projector_tiles(const double *W, int D, std::vector<cd> &A, std::vector<cd> &B) {
    A.assign((size_t)D * D, cd{0.0, 0.0});
    B.assign((size_t)D * D, cd{0.0, 0.0});
    for (int i = 0; i < D; ++i) {
        A[(size_t)i * D + i] = cd{W[i], 0.0};
        B[(size_t)i * D + i] = cd{W[i] != 0.0 ? 1.0 : 0.0, 0.0};
    }
}

// Sectors: connected components of the union sparsity pattern of every operator H0 uses
// (the levels an evolution can ever couple).  A single level with a zero diagonal in every
// operator never evolves (its propagator is 1 and it carries no gradient): it is "fixed" and
// only enters the head's U.  A single level with a diagonal entry evolves by a phase of its own; when
// it is idle (idle_levels: no projector weight, no target entry beside its diagonal) that phase reaches
// neither F nor any derivative -- every term of the heads carries P0 or its pattern on both sides of
// K = U0^dag U, block diagonal there -- and the level is left out altogether (the dark state
// (|1r> - |r1>) / sqrt 2 of the detuned d = 9 Rydberg model: as a third, padded 2-level sector it kept
// the plan off the pair, merged and one-workgroup kernels).  The others are packed first-fit-decreasing into sectors of
// S = max(2, largest component) slots -- one class -- or, when that costs at least a quarter
// less work (sum of nsec S^3), into two classes: the components above a size cut in sectors of
// their largest size, the rest in sectors of theirs (d = 9 Rydberg: one sector of 4 and two of
// 2 instead of two of 4).  sidx[w * S + a] = level in slot a of sector w, or -1 (padding: a
// decoupled level, exp(0) = 1, never reaches F).  Only for operator-basis plans (the pattern
// covers H0's and the error sources' operators), and only when the sector work is at most half
// of d^3.
struct SectorClass {
    int S = 0, nsec = 0;
    std::vector<int> sidx;
};
struct SectorSetup {
    std::vector<SectorClass> cls;
    std::vector<int> fixed;
};
static SectorClass pack_sectors(const std::vector<std::vector<int>> &comps) {  // comps sorted by size, desc
    SectorClass sc;
    sc.S = std::max(2, (int)comps[0].size());
    std::vector<std::vector<int>> bins;
    for (const auto &c : comps) {
        bool placed = false;
        for (auto &bn : bins)
            if ((int)(bn.size() + c.size()) <= sc.S) {
                bn.insert(bn.end(), c.begin(), c.end());
                placed = true;
                break;
            }
        if (!placed) bins.push_back(c);
    }
    sc.nsec = (int)bins.size();
    sc.sidx.assign((size_t)sc.nsec * sc.S, -1);
    for (int w = 0; w < sc.nsec; ++w)
        for (size_t a = 0; a < bins[w].size(); ++a) sc.sidx[(size_t)w * sc.S + a] = bins[w][a];
    return sc;
}
static long sector_cost(const SectorClass &c) { return (long)c.nsec * c.S * c.S * c.S; }
static SectorSetup find_sectors(const grape_desc *desc, bool tables, const std::vector<char> *idle = nullptr) {
    SectorSetup ss;
    const int D = desc->ndim;
    if (tables || D > GRAPE_MAX_SMALL_DIM || (desc->reserved[1] & GRAPE_OPT_NO_SECTORS)) return ss;
    std::vector<int> parent(D);
    for (int i = 0; i < D; ++i) parent[i] = i;
    auto root = [&](int i) {
        while (parent[i] != i) i = parent[i] = parent[parent[i]];
        return i;
    };
    // every operator the propagators use: H0's and the error sources'
    std::vector<int> used;
    for (int t = 0; t < desc->n_h0_terms; ++t) used.push_back(desc->h0_terms[t].op);
    const int n_err_terms = desc->nerr > 0 ? desc->err_term_offsets[desc->nerr] : 0;
    for (int t = 0; t < n_err_terms; ++t) used.push_back(desc->err_terms[t].op);
    std::vector<char> diag(D, 0);  // level with a nonzero diagonal entry in some operator
    for (int o : used) {
        const double *op = desc->ops + 2 * (size_t)o * D * D;
        for (int c = 0; c < D; ++c)
            for (int r = 0; r < D; ++r) {
                const double *v = op + 2 * ((size_t)r + (size_t)c * D);
                if (v[0] == 0.0 && v[1] == 0.0) continue;
                parent[root(r)] = root(c);
                if (r == c) diag[r] = 1;
            }
    }
    std::vector<std::vector<int>> comps;
    std::vector<int> slot(D, -1), fixed;
    for (int i = 0; i < D; ++i) {  // levels in ascending order inside each component
        const int r = root(i);
        if (slot[r] < 0) {
            slot[r] = (int)comps.size();
            comps.emplace_back();
        }
        comps[slot[r]].push_back(i);
    }
    const size_t ncomp = comps.size();
    comps.erase(std::remove_if(comps.begin(), comps.end(),
                               [&](const std::vector<int> &c) {
                                   if (c.size() != 1) return false;
                                   if (diag[c[0]]) return idle && (*idle)[c[0]] != 0;  // (left out: not fixed)
                                   fixed.push_back(c[0]);
                                   return true;
                               }),
                comps.end());
    if (ncomp < 2 || comps.empty()) return ss;
    std::stable_sort(comps.begin(), comps.end(),
                     [](const std::vector<int> &a, const std::vector<int> &b) { return a.size() > b.size(); });
    std::vector<SectorClass> best{pack_sectors(comps)};
    long cost = sector_cost(best[0]);
    for (size_t i = 1; i < comps.size(); ++i) {
        if (comps[i].size() == comps[i - 1].size()) continue;
        const std::vector<std::vector<int>> a(comps.begin(), comps.begin() + i), b(comps.begin() + i, comps.end());
        std::vector<SectorClass> two{pack_sectors(a), pack_sectors(b)};
        const long c2 = sector_cost(two[0]) + sector_cost(two[1]);
        if (4 * c2 <= 3 * cost) {
            best = two;
            cost = c2;
        }
    }
    if (2 * cost > (long)D * D * D) return ss;
    for (const auto &c : best)
        if (c.nsec * c.S * c.S > grape_proj::kSectorLds) return ss;
    if (best.size() == 1 && best[0].nsec < 2 && fixed.empty()) return ss;
    ss.cls = best;
    ss.fixed = fixed;
    return ss;
}

}  // namespace grape_setup
