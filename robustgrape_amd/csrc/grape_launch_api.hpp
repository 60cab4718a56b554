// grape_launch_api.hpp -- what the host units (grape_plan.hpp) and the other engines' API headers see of the
// small-d engine's launch sequences: its plan-time constants, the profiling mark, the list of compiled
// dimensions, and the DECLARATIONS of the function templates that grape_launch.hpp defines.  No body and no
// kernel header: a unit that includes only this cannot instantiate a kernel, and a launch sequence that no
// kernel unit instantiates (grape_inst.hip, grape_prod_inst.hip) is a link error.
#pragma once
#include <hip/hip_runtime.h>

#include "grape.h"
#include "grape_types.hpp"

namespace grape_host {

using grape::cd;
using grape::DevBatch;
using grape::DevProblem;

// Scan workgroups: one per evaluation, W waves of row groups.  W = 8 (52 chunks
// of L = 10 steps at d = 9, N_t = 512) has the shortest chains; W = 4 halves
// the LDS and registers per block so two evaluations share a CU, which wins
// once there are more evaluations than CUs (plan-time choice, see kScanWide).
// Sector problems with many sub-evaluations per CU take W = 1: fewer chunks mean
// fewer carries and per-chunk images to stream (C2 2.69 -> 2.80 M evals/s).
constexpr int kScanWide = 8, kScanNarrow = 4, kScanTiny = 1;
// Latency-bound calls (fewer sub-evaluations than CUs: single evaluations, C4's 32 restarts per
// GPU, the optimiser's tail rounds) of the chunk-walk classes (<= kWalkMaxD levels, no error
// sources) take 16-wave scans: twice the chunks of kScanWide, so each walk lane steps half as far
// (L = 2 at 4 levels, L = 1 at 2 levels for N_t = 512).
constexpr int kScanLatency = 16;

// Lane-matrix exponentials (grape_lane.hpp k_expm_lane) for d <= kLaneMaxD (operator-basis
// builders; closure tables keep k_expm_table); GRAPE_OPT_NO_LANE selects the row-group k_expm (A/B and
// the bit-identity test).  Measured per instantiation (C2 sectors, 32 768 evaluations per pass,
// rocprof, one box, profiles/r02/lane): S = 2 k_expm 1.057 -> 0.957 ms; S = 4 1.99 -> 2.26 ms (a
// 4 x 4 complex matrix per lane is 64 VGPRs: 2 waves/SIMD), so d = 4 keeps the row groups.
constexpr int kLaneMaxD = 3;
// Sector stage 0 without error sources: propagators and chunk chains per lane up to kChainMaxD
// (k_expm_chain_lane; a d = 4 variant measured 7.32 vs 3.81 ms and was dropped, grape_lane.hpp);
// GRAPE_OPT_NO_CHAIN keeps k_expm + k_scan.  (Both are the fallbacks of the chunk walks,
// grape_walk.hpp, which serve these classes by default.)
constexpr int kChainMaxD = kLaneMaxD;

// Optional per-kernel event marks (profiling mode): fn(ctx, kernel, 0|1) around each launch.
struct KMark {
    void *ctx = nullptr;
    void (*fn)(void *, int, int) = nullptr;
    void operator()(int k, int phase) const {
        if (fn) fn(ctx, k, phase);
    }
};

// the compiled dimensions: one grape_inst.hip / grape_prod_inst.hip unit each (build.DIMS)
#define GRAPE_DIMS(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)

// Defined in grape_launch.hpp, instantiated per dimension in grape_inst.hip.
template <int D>
hipError_t launch_pipeline(const DevProblem &P, const DevBatch &B, const grape::FactorTab &F, hipStream_t st,
                           const KMark &mark);
template <int D>
hipError_t launch_sector_stage(int stage, const DevProblem &P, const DevBatch &B, const grape::FactorTab &F,
                               hipStream_t st, const KMark &mark);
template <int D>
hipError_t launch_sector_reduce(const DevProblem &P, const DevBatch &B, const grape::SecParts &S, int nev,
                                hipStream_t st, const KMark &mark);
template <int D>
hipError_t launch_expm_raw(const cd *A, cd *E, int n, int *ovf, int *ovf_count, int *status, int *mstats,
                           hipStream_t st);
template <int D>
hipError_t set_lds_limits();
template <int D>
hipError_t launch_expm_variants(const DevProblem &P, const DevBatch &B, const grape::FactorTab &F, hipStream_t st);
template <int D>
hipError_t launch_expm_table(const DevProblem &P, const DevBatch &B, hipStream_t st);
// <4, 2> and <3, 2> at W = kScanLatency and kScanTiny: grape_inst.hip's units of D0
template <int D0, int D1, int W = kScanLatency>
hipError_t launch_scan_pair(const DevProblem &P0, const DevBatch &B0, const DevProblem &P1, const DevBatch &B1,
                            hipStream_t st);

// Product coefficients (grape_prod.hpp): plans with factor terms (F.h0 set) run k_expm_prod / k_expm_grad_prod
// wherever the launch sequences launch k_expm / k_expm_grad.  Defined and instantiated per dimension in
// grape_prod_inst.hip; the launch geometry is that of the plain kernels.
template <int D>
hipError_t launch_expm_prod(bool err, const DevProblem &P, const DevBatch &B, const grape::FactorTab &F, hipStream_t st);
template <int D>
hipError_t launch_expm_grad_prod(const DevProblem &P, const DevBatch &B, const grape::FactorTab &F, hipStream_t st);

}  // namespace grape_host
