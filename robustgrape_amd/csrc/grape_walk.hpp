// grape_walk.hpp -- chunk walks: the sector pipeline without HBM intermediates (round 3).
//
// For sector classes of D <= kWalkMaxD levels without error sources (the Rydberg sectors of
// 4 and 2 levels), ONE LANE OWNS ONE (sub-evaluation b', chunk c) and walks the chunk's
// steps twice:
//
//   k_walk_fwd   E_k = exp(A_k) and the chunk chain Q <- E_k Q, in registers; writes only
//                the chunk total T_c (k_scan then scans the totals: B.Tc).
//                                                     UnitaryCalculations.jl:45-47,99
//   k_walk_grad  X = M'_c = Carry_c M Carry_c^dag (formed in the lane) and per step
//                  E_k again, Y_k = X E_k^dag, and for every gradient parameter u the
//                  eps-variant E'_k contracted on the spot,
//                  F_dx[u,k] = Re tr(Y_k (E'_k - E_k)/eps)    (FidelityCalculations.jl:56-76),
//                  then X <- E_k Y_k.
//
// Algebra (grape_kernels.hpp): F_dx[u,k] = Re tr(C_{k-1} M C_k^dag dE_{k,u}) with
// C_k = E_k C_{k-1}, so with X_{k-1} = C_{k-1} M C_{k-1}^dag (= M'_c at a chunk start) the
// gradient kernel of step k is Y_k = X_{k-1} E_k^dag and X_k = E_k X_{k-1} E_k^dag = E_k Y_k.
// The nominal propagator is recomputed in the second walk instead of being stored: at 4
// levels one exponential costs ~1.2 k FMAs per lane, storing and re-reading it 512 B of HBM
// traffic, and the round-2 pipeline moved 1.08 MB of E / Q intermediates per evaluation.
//
// Arithmetic.  A = -i dt H is skew-Hermitian (grape_plan_create checks that H0's terms are
// Hermitian), A^2 Hermitian and A^3 skew-Hermitian, so each is kept COMPRESSED: its diagonal
// (the imaginary / real parts) and strict upper triangle -- 16 instead of 32 doubles at D = 4,
// and every product with a diagonal entry is 2 FMAs instead of 4.  The exponential is the
// row-group kernels' solve-free Taylor evaluation (Paterson-Stockmeyer in A^3; degree 12, 9 or 6
// by the |re|+|im| column bound of A shifted by the midpoint of its diagonal, sm_regime), column
// by column: column i of exp(A) needs
// only column i of A, A^2 and the running vector, so no full matrix is materialised for it.
// Above the Taylor-12 range (exact 1-norm > 0.25) the lane takes Taylor 30 of A / 2^s with
// |A / 2^s|_1 <= 3.2 and squares s times (Higham's scaling and squaring; kWalkThetaHi) -- where
// the row-group path parks the item for Julia's Pade 7 / 9 / 13, with the same measured accuracy.  Both are
// exp(A) to a few ulps (T0); the FD differences keep the reference's (E' - E) / eps form,
// element by element, before the contraction.
//
// Registers (D = 4): X 64 VGPRs across the walk, the A / A^2 / A^3 set 96, one vector of
// temporaries; in k_walk_grad<4> X / Y live in the lane's private LDS slot (17 complex, padded so
// that the 16-B reads of 16 lanes hit 64 distinct banks).  The walks are compiled in their own
// translation unit (grape_walk_inst.hip) without MachineLICM: hoisting the trig / log
// polynomial constants of the inlined ocml calls out of the step loop pinned ~50 VGPRs and
// spilled the walk state (k_walk_grad<2>: 128 VGPRs + 18 spilled -> 98, none spilled).
//
// This file is the umbrella: the kernels live in six pieces, one per family, included in this order
// (grape_walk_inst.hip instantiates all of them in ONE translation unit: DESIGN.md 10 says why).
//   grape_walk_core.hpp    the column exponential and the term builder, MStore, the lane geometry, the knobs
//   grape_walk_gauge.hpp   phase-covariant helpers: charges, gauge_cis, pair phases, FD weights, E~
//   grape_walk_chunk.hpp   k_walk_fwd, k_walk_grad and the pair kernels
//   grape_walk_merged.hpp  k_gauge_base_fill, k_walk_fwd_m / k_walk_grad_m (matrix, rank-one, wide), k_scan_seq
//   grape_walk_img.hpp     k_walk_img, k_walk_img_gauge, k_walk_img_sum, k_walk_err_grad
//   grape_walk_lab.hpp     k_gauge_err_base_fill, k_walk_wsum_lab, k_walk_err_lab
// Every piece compiles on its own (tests/test_capi_cpu.py); the last four need only core and gauge.
#pragma once
#include "grape_walk_core.hpp"
#include "grape_walk_gauge.hpp"
#include "grape_walk_chunk.hpp"
#include "grape_walk_merged.hpp"
#include "grape_walk_img.hpp"
#include "grape_walk_lab.hpp"
