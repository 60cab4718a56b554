// grape_types.hpp -- the plain data every layer shares: the complex element, the term and variant records,
// and the problem / batch descriptors that the host units fill and every kernel takes by value.
// No device code and no HIP header: plain C++17, so that the host logic on a descriptor
// (grape_plan_setup.hpp, grape_descriptor.hip) compiles, links and is tested without the kernels.
// The kernel headers (grape_device.hpp, grape_kernels.hpp) and every *_api.hpp include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace grape {

struct cd {
    double re, im;
};

struct Term {  // layout-identical to grape_term (include/grape.h)
    int32_t op, var, index, func;
    double a, b, sre, sim;
};

enum { VAR_ONE = 0, VAR_X = 1, VAR_XADD = 2, VAR_TSTEP = 3 };
enum { FN_ONE = 0, FN_LINEAR = 1, FN_COS = 2, FN_SIN = 3, FN_CIS = 4 };

struct Pert {
    int var;      // -1: none
    int index;
    double delta;
};

// One propagator variant of a time step: the closure call sites of
// UnitaryCalculations.jl:45-90 (perturb one variable by delta; optionally add
// the error Hamiltonian e with strength errval).
struct VSpec {
    Pert pert;
    int err;        // -1: none
    double errval;
};

// Product coefficients (grape.h GRAPE_OP_FACTOR): the factor terms of every operator term of P.h0 and of
// P.err, kMaxFactors slots per operator term in the lists' order.  A slot's op is 1 when it holds a factor
// and 0 when it is empty; its value scale * f(a v + b) is real.  Plans without factor terms have h0 = null.
// An argument of its own of the product kernels (grape_prod.hpp), not a field of DevProblem: every kernel
// takes that by value.
constexpr int kMaxFactors = 2;  // GRAPE_MAX_FACTORS
struct FactorTab {
    const Term *h0;   // [n_h0][kMaxFactors]
    const Term *err;  // [err_off[ne]][kMaxFactors]
};

// Everything a kernel needs to know about the problem (passed by value).
struct DevProblem {
    int D, Nt, np, na, ne, nx;
    int nv;              // propagator variants per step (nominal + FD variants)
    int n_h0, n_tgt;
    int xadd_dep;        // H0 depends on x_add -> x_add FD variants exist
    int L, nchunks;      // scan chunking
    int scan_waves;      // waves per k_scan / k_err_scan workgroup (4 or 8)
    // variant layout (see grape_plan_setup.hpp: build_variants)
    int off_dx, off_dxa, off_dx2, off_err, err_stride;
    int nvg, nz;         // gradient parameters (np + x_add when xadd_dep); local-frame slots per step (error path)
    double dt, eps, eps2, inv_eps, inv_eps2sq, DD, Dtr;
    const cd *ops;       // [n_ops][D][D] row-major
    const cd *opsT;      // [n_ops][D][D] column-major (column builds for the exp kernels)
    const Term *h0;
    const Term *tgt;
    const Term *err;     // error-source terms
    const int *err_off;  // [ne+1]
    const VSpec *vs;     // [nv]
    const double *W;     // projector diagonal (weights)
    // general (non-diagonal or complex) projector P0: the diagonal-specialised results are
    // overwritten by the heads of grape_projector.hip (FidelityCalculations.jl:47-51)
    int gen_proj;
    const cd *PA;        // P0 P  (row-major), P = P0 with nonzeros set to 1
    const cd *PB;        // P     (row-major)
    const cd *P0g;       // P0    (row-major; expectation values)
    // Sectors (grape_plan_setup.hpp find_sectors): when every operator H0 uses is block-diagonal in
    // a common permutation, one evaluation is run as nsec independent D x D sector problems
    // (sub-evaluation b' = b * nsec + w reads x of b and the operators of sector w at
    // ops / opsT + w * sec_ops); k_scan stops after the chunk carries, the sector head
    // (grape_projector.hip) forms F and the blocks of M from the assembled U, and k_sec_mc the
    // per-chunk images M'_c.  sectors = 0: whole matrices (nsec = 1).
    int sectors;         // 1: this is the sector problem (k_scan stops after the carries)
    int nsec;
    size_t sec_ops;
    int walk;            // sector class served by the chunk walks (grape_walk.hpp: k_walk_fwd / k_walk_grad)
    int walk_store_e;    // ... k_walk_fwd stores the nominal propagators for k_walk_grad (B.Ew) instead of
                         //     k_walk_grad recomputing them
    int twin;            // ... two sectors with identical operator blocks (grape_walk.hpp TWIN): one
                         //     exponential per step serves both
    int opts;            // grape_desc.reserved[1]: GRAPE_OPT_* (fixed at plan creation)
    // Phase-covariant walk class (grape_walk.hpp GAUGE, round 5): every sector w of the class obeys
    // H_w(x) = D(a x) H_w(0) D(a x)^dag with D(t) = diag(e^{i t N_j}) for the one control x (np = 1,
    // H0 free of x_add and of the step index), so E_k = D_k E~ D_k^dag with E~ = exp(-i dt H_w(0))
    // and the eps-variant is E' = D'_k E~ D'_k^dag: one exponential per lane instead of one per step
    // and variant.  gauge_n: [nsec][D] the integer charges N_j >= 0 (engine: find_gauge).
    int gauge;
    double gauge_a;
    const int *gauge_n;
    // (round 6) every sector of the class has the ladder charges N_j = j (the Rydberg sectors in the
    // engine's level order: {11, S, rr} and {01, 0r}): the merged walks then take the pair phases and
    // difference weights from compile-time charge differences (grape_walk.hpp kLadder), same values
    int gauge_ladder;
    // (round 6) E~ of every sector of the class, [nsec][D][D] row-major, computed once at plan creation by
    // the walks' own exponential (grape_walk.hpp k_gauge_base_fill: the same bits as gauge_base_lds) for
    // the merged walks, which read it through scalar loads (SGPR operands) instead of LDS copies
    // With error sources (gauge_lab, round 6): the lab-frame error walks (grape_walk.hpp k_walk_wsum_lab /
    // k_walk_err_lab, no images) and gauge_Et = [nsec][1 + 2 ne][D][D]: E~, N_e = (E~_e1 - E~) / eps,
    // M_e = E~_e2 - E~ (k_gauge_err_base_fill)
    const cd *gauge_Et;
    int gauge_lab;
    // Rank-one merged gradient walk (grape_walk.hpp merged_step_grad_r1): with the diagonal head and exactly one
    // projector-weighted level per sector, every sector's M block is e_c m^T, so the walk carries two vectors
    // per sector.  rank1_c[w]: that level's in-sector index c of sector w (launch-uniform; addresses only).
    int rank1;
    int rank1_c[2];
};

struct DevBatch {
    int nb;                 // evaluations in this launch
    const double *x;        // [nb][nx]
    cd *E;                  // [nb][Nt][nv][D][D]
    cd *Q;                  // [nb][Nt][D][D]
    cd *Mc;                 // [nb][nchunks][D][D]
    double *F;              // [nb]
    double *Fdx;            // [nb][nx]
    double *part_add;       // [nb][Nt][na]   (xadd_dep only)
    double *tgt_part;       // [nb][na]
    cd *Carry;              // [nb][nchunks][D][D]  C_{cL-1} (identity for c = 0)
    cd *Ub;                 // [nb][D][D]           U = C_Nt
    cd *Me;                 // [nb][ne][nchunks][3][D][D]  M'_{c,e}, T_c, Ttot_c (error path)
    cd *Wc;                 // walk path with error sources: [nb][ne][nchunks][D][D] chunk sums of W (k_walk_img_sum)
    cd *Zl;                 // [nb][Nt][nz][D][D]  local-frame differences (error path, k_err_local):
                            //   Z1_u (nvg) | W_e (ne) | Z2_{e,u} (ne x nvg), row-major
    double *Fd2;            // [nb][ne]
    double *Fd2dx;          // [nb][ne][nx]
    double *part_err_add;   // [nb][ne][Nt][na]  per-step x_add terms of F_d2err_dx (xadd_dep only)
    int *overflow;          // parked (Pade m > 5) item ids of k_expm
    int *overflow_count;
    int *ovf2;              // parked item ids of k_expm_grad
    int *ovf2_count;
    cd *ovf2_slots;         // [nb][Nt][nvg][D][D]  A of parked k_expm_grad items
    int *status;            // bit 0: singular Pade denominator
    cd *sink;               // [D][D] write-only target of inactive lanes' unconditional stores
    // closure fallback (grape_fidelity_grad_tables): host-evaluated closures, per evaluation
    const cd *Htab;         // [nb][Nt][nv][D][D] column-major H at every closure call site (else null)
    const cd *U0tab;        // [nb][1 + na][D][D] column-major target at x_add, x_add + eps e_q (else null)
    cd *gp_scr;             // general projector: head scratch (grape_projector_api.hpp)
    double *sec_part;       // sectors: [nb][Nt][nvg] per-sector F_dx terms (k_sec_reduce sums them), else null;
                            // chunk walks: [nsec][Nt][nvg][nb / nsec], the evaluation fastest (coalesced)
    const cd *Msec;         // sectors: [nb][D][D] the sector blocks of M = G U (the sector head)
    // sectors with error sources
    double *sec_part_err;   // [nb][ne][Nt][nvg] per-sector F_d2err_dx terms (k_sec_reduce_err sums them)
    cd *TotS;               // [nb][ne][D][D] the sector blocks of Tot = sum_k V^err_k (k_err_scan)
    const cd *MsecE;        // [nb][ne][D][D] the sector blocks of M_e = G_e U (the sector error head)
    int chains_done;        // k_scan: Phase A's chunk chains Q_k are already in Q (k_expm_chain_lane);
                            //   a chunk whose total holds a NaN (a parked step) is rechained from E
    // chunk walks (grape_walk.hpp): k_scan starts from the chunk totals in Tc when it is set
    cd *Tc;                 // [nb][nchunks][D][D] row-major chunk totals T_c (k_walk_fwd), else null
    cd *wscr;               // [nsec][nb / nsec][nchunks][2][D][D] per-lane scratch of the squaring path
    cd *Ew;                 // walk_store_e: [nsec/NS][L][NS][D*D + 1][lanes] shifted E~_k and its shift, lane-minor
};

// Sectors: F_dx[b][k, u] (or the per-step x_add term) = sum over the evaluation's sectors of
// both classes, in sector order (deterministic).  A class's terms are laid out per evaluation
// ([nb][nsec][Nt][nvg]) or, from the chunk walks, evaluation-fastest ([nsec][Nt][nvg][nb])
// (grape_kernels.hpp k_sec_reduce).
struct SecParts {
    const double *part[2];      // per sector class, layout by lane_major
    const double *part_err[2];  // per sector class (error sources), layout by lane_major_err
    int nsec[2];                // 0 for an absent class
    int lane_major[2];          // 1: [nsec][Nt][nvg][nb] (chunk walks), else [nb][nsec][Nt][nvg]
    int lane_major_err[2];      // 1: [nsec][ne][Nt][nvg][nb] (k_walk_err_grad), else [nb][nsec][ne][Nt][nvg]
};

}  // namespace grape

// Two capacities that a host validator and a kernel must agree on live here, in their engines' namespaces,
// so that the validator (find_sectors, validate_desc) reads them without the engine's launch header.
namespace grape_proj {
constexpr int kSectorLds = 2048;  // complex elements of LDS for the sector blocks M_ww (nsec * S * S)
}
namespace grape_tiled {
constexpr int kMaxTerms = 256;  // H0 / target terms a tiled plan serves (coefficients staged in LDS)
}
