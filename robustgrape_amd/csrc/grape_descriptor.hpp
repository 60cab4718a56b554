// grape_descriptor.hpp -- what the descriptor unit (grape_descriptor.hip: pure host logic on a grape_desc)
// hands to the units that build a plan from it: the factor split, the projector and symmetry setups, the
// route, and the declarations of its functions.  Private to the library's host units (not installed).
#pragma once
#include <string>
#include <vector>

#include "grape.h"
#include "grape_plan_setup.hpp"
#include "grape_symmetry.hpp"

using grape::cd;

namespace grape_eng {

// sets the calling thread's grape_last_error() message and returns `code` (grape_engine.hip)
int fail(int code, const std::string &msg);

// (SectorClass, SectorSetup, pack_sectors, sector_cost and find_sectors -- the layout rule -- live in
// grape_plan_setup.hpp, where tests/c/descriptor_check.cpp runs them on the host.)
using grape_setup::SectorClass;
using grape_setup::SectorSetup;
using grape_setup::find_sectors;
using grape_setup::pack_sectors;
using grape_setup::sector_cost;

// Product coefficients (grape.h GRAPE_OP_FACTOR).  A validated descriptor split once into the plain
// descriptor every other piece of host logic sees -- operator terms only, err_term_offsets re-based, so
// that nothing ever indexes ops[-1] -- and the factor slots of its H0 and error terms
// (grape_types.hpp FactorTab: kMaxFactors slots per operator term, op = 1 live, 0 empty).  A descriptor
// without factor terms is passed through untouched (plain = *desc, the caller's own pointers).
struct FactorSplit {
    bool any = false;
    bool reads_xadd = false, reads_tstep = false;  // some factor reads x_add / the step index
    grape_desc plain{};
    std::vector<grape_term> h0, err, fac_h0, fac_err;
    std::vector<int32_t> err_off;
};

// The projector (FidelityCalculations.jl:47-51): the full matrix P0 when given, else its
// diagonal.  A real diagonal P0 is served by the engines' specialised kernels (weights W);
// anything else sets gen_proj and keeps A = P0 P, B = P (P = P0 with nonzeros set to 1)
// and P0 itself, row-major, for the general heads (grape_projector.hip).
struct ProjectorSetup {
    std::vector<double> W;
    std::vector<cd> A, B, P0;
    bool general = false;
    double trP = 0.0;
    void set_general(int D, const std::vector<cd> &pattern) {  // B = the pattern P, A = P0 P
        std::fill(W.begin(), W.end(), 0.0);  // the specialised results are all overwritten
        B = pattern;
        A.assign((size_t)D * D, cd{0.0, 0.0});
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j)
                for (int l = 0; l < D; ++l) {
                    const cd a = P0[(size_t)i * D + l], b = B[(size_t)l * D + j];
                    A[(size_t)i * D + j].re += a.re * b.re - a.im * b.im;
                    A[(size_t)i * D + j].im += a.re * b.im + a.im * b.re;
                }
    }
};

// Symmetry-adapted sectors (grape_symmetry.hpp): the sector path's view of the problem in the basis
// V that splits the sparsity components further -- every operator V^dag O V (grape_desc layout;
// H0's and the error sources' operators with their off-block residue set to exact zeros, the others
// with rounding residue below 1e-15 of their largest entry snapped to 0), and the head's projector:
// P0' = V^dag P0 V with the pattern P' = V^dag P V of the ORIGINAL P0 (P = P0 .!= 0,
// FidelityCalculations.jl:47-51 -- the pattern of P0' is not P' in general).  On only when the
// rotated sectors cost less work (sum nsec S^3) than the permutation sectors.
struct SymSetup {
    bool on = false;
    grape_sym::Split split;
    std::vector<double> ops;  // n_ops * d * d complex, column-major interleaved
    ProjectorSetup ps;        // the rotated projector (A = P0' P', B = P' when not diagonal)
    grape_desc view(const grape_desc *d) const {
        grape_desc v = *d;
        v.ops = ops.data();
        return v;
    }
};

// Which engine serves the descriptor (pure host logic).
struct Route {
    bool tables = false;      // GRAPE_DESC_HOST_TABLES: host-evaluated H and target tables
    bool general_h0 = false;  // the general path (materialised derivatives, LU inverse of the chain)
    bool pivot = false;       // ... over the dense engine's pivoted exponential (12 < d <= 64)
    bool xadd_dep = false;    // H0 or an error source reads x_add: x_add variants exist
    bool err_herm = true;     // Hermitian error generators
};

// grape_descriptor.hip
void split_factors(const grape_desc *desc, FactorSplit &fs);
int check_hermitian_terms(const grape_desc *desc, const grape_term *t, int n, const char *what);
ProjectorSetup setup_projector(const grape_desc *desc);
std::vector<char> idle_levels(const grape_desc *desc, const grape_desc &sdesc, const ProjectorSetup &sps);
bool find_gauge(const grape_desc *desc, const grape_desc &sdesc, const SectorClass &sc, double &a,
                std::vector<int> &N);
SymSetup symmetry_setup(const grape_desc *desc);
int validate_desc(const grape_desc *desc, int *n_err_terms);
int choose_route(const grape_desc *desc, int n_err_terms, Route &rt);

}  // namespace grape_eng
