// grape_walk_api.hpp -- host launchers of the chunk walks (grape_walk.hpp), compiled in their own
// translation unit (grape_walk_inst.hip, built without MachineLICM; see grape_walk.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "grape_types.hpp"

namespace grape {
constexpr int kWalkMaxD = 4;  // sector classes of at most this many levels take the walks
constexpr int kWalkMaxNpA = 2;  // ... with at most this many controls per step and x_add entries
constexpr int kGaugeMaxE = 8;  // error sources of a phase-covariant image walk (grape_walk.hpp k_walk_img_gauge)
constexpr int kWalkBlockA = 128;  // lanes per workgroup (grape_walk.hpp kWalkBlock)
// walk classes of at least this many levels hand the forward walk's propagators to the gradient walk
// (B.Ew) instead of recomputing them (the engine's P.walk_store_e and the launchers agree on it)
constexpr int kWalkStoreMinD = 4;
// The walks read the controls row-major from x itself (stride 1 per value, nx per evaluation; no transposed
// copy).  Each lane streams its own row: 8 steps per 64-B line, reused from the vector cache.
// error sources on a phase-covariant class (round 6): the lab-frame walks k_walk_wsum_lab / k_walk_err_lab
// (grape_walk.hpp; the engine's P.gauge_lab), no images.  0: the image walk and its back end (A/B)
#ifndef GRAPE_WALK_ERR_LAB
#define GRAPE_WALK_ERR_LAB 1
#endif
constexpr int kLabBaseMaxLanes = 256;  // k_gauge_err_base_fill: one lane per (sector, base matrix)
}  // namespace grape

namespace grape_walk {
// one lane per (sector, evaluation, chunk) of the class: stage 0 = k_walk_fwd (chunk totals to
// B.Tc), stage 1 = k_walk_grad (per-sector F_dx terms to B.sec_part, evaluation-fastest).  With
// error sources (P.ne > 0, nvg == 1): stage 0 = k_walk_img (chunk totals and the lane-minor
// local-frame images to B.Zl), stage 1 = k_walk_img_sum (per-sector F_dx terms to B.sec_part,
// lane-major, and the chunk sums of W to B.Wc), stage 2 = k_walk_err_grad (per-sector F_d2err_dx
// terms to B.sec_part_err, lane-major).  Phase-covariant classes with error sources (P.gauge_lab): stage 0 =
// k_walk_wsum_lab (chunk totals and the chunk sums of W to B.Wc), stage 1 = nothing, stage 2 =
// k_walk_err_lab (F_dx and F_d2err_dx terms, lane-major), no images
template <int D>
hipError_t launch(int stage, const grape::DevProblem &P, const grape::DevBatch &B, hipStream_t st);
// Latency-bound calls of the Rydberg layout -- class 0: one 4-level sector (permutation sectors) or
// one 3-level sector (symmetry-adapted), class 1: two 2-level sectors, no error sources, one gradient
// parameter -- run both classes' walks
// of a stage in ONE launch (k_walk_fwd_pair / k_walk_grad_pair).  pair_ok tells whether the layout
// fits; launch_pair(stage, ...) then replaces launch<4>(stage, class 0) + launch<2>(stage, class 1).
bool pair_ok(const grape::DevProblem &P0, const grape::DevProblem &P1);
hipError_t launch_pair(int stage, const grape::DevProblem &P0, const grape::DevBatch &B0, const grape::DevProblem &P1,
                       const grape::DevBatch &B1, hipStream_t st);
// Throughput passes of the same layout with phase-covariant classes at equal chunking: ONE lane walks
// both classes of an (evaluation, chunk) (k_walk_fwd_m / k_walk_grad_m); the gradient stage writes
// one F_dx part, the sum of the two classes' (either order gives the same double), into class A's
// sec_part.  Stage 0: k_walk_fwd_m (chunk totals, lane-minor), stage 2: k_scan_seq (carries and U
// from them), stage 1: k_walk_grad_m, which writes the F_dx rows itself (no k_sec_reduce for such passes).
// merged_ok tells whether the classes fit.
bool merged_ok(const grape::DevProblem &PA, const grape::DevProblem &PB);
// 1: the merged gradient walk carries one summed state for a twin class's two sectors (GRAPE_WALK_TWIN_SUM)
bool merged_twin_sum();
// E~ of the class's nsec sectors into out [nsec][D][D] (DevProblem::gauge_Et; scr: 2 D^2 complex per sector)
hipError_t fill_gauge_base(const grape::DevProblem &P, int nsec, grape::cd *scr, grape::cd *out, hipStream_t st);
// the lab-frame error walks' base table [nsec][1 + 2 ne][D][D] (DevProblem::gauge_Et with gauge_lab; scr: 2 D^2
// complex per base matrix)
hipError_t fill_gauge_err_base(const grape::DevProblem &P, int nsec, grape::cd *scr, grape::cd *out, hipStream_t st);
hipError_t launch_merged(int stage, const grape::DevProblem &PA, const grape::DevBatch &BA, const grape::DevProblem &PB,
                         const grape::DevBatch &BB, hipStream_t st);
// The wide pass of a rank-one merged plan (grape_walk.hpp, "The wide pass"): one lane per evaluation over all
// N_t steps, BA.nb evaluations, no chunks and no scan.  Stage 0: k_walk_fwd_m<..., WIDE> walks psi = U e_c forward
// and writes psi_N (BA.Ub / BB.Ub: entry j of chain ch at [(ch * D + j) * nb + b], twins one chain); stage 1:
// k_walk_grad_m<..., WIDE> starts from it and the head's alpha per sector (BA.Msec / BB.Msec: [nb * nsec], WideHead) and walks
// back in time, writing the F_dx rows.  Both read BA.x ([nb][nx], no transposed copy) through workgroup tiles of
// 16 steps.  wide_ok tells whether the classes fit.
constexpr int kWideMaxNt = 4096;
bool wide_ok(const grape::DevProblem &PA, const grape::DevProblem &PB);
hipError_t launch_merged_wide(int stage, const grape::DevProblem &PA, const grape::DevBatch &BA, const grape::DevProblem &PB,
                              const grape::DevBatch &BB, hipStream_t st);
// F_dx parts the class's gradient stage writes per evaluation: its sectors, or (k_walk_grad with several
// sectors per lane, no error sources) one pre-summed part per lane row (grape_walk.hpp walk_grad_body)
int grad_parts(const grape::DevProblem &P);
}  // namespace grape_walk
