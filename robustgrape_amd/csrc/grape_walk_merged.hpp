// grape_walk_merged.hpp -- both sector classes of the Rydberg layout in one lane (a piece of grape_walk.hpp):
// k_gauge_base_fill (the plan's E~ tables), the merged forward and gradient walks k_walk_fwd_m / k_walk_grad_m
// in their three forms -- the matrix walk (merged_step_grad), the rank-one walk (merged_step_grad_r1) and the
// wide pass without time chunks (wide_*; the WIDE flag of the same two kernels) -- and k_scan_seq, the scan of
// their chunk totals.  This is where the C2 metric is made; the kernels are register-tight (222 VGPRs in the
// matrix gradient walk), and their code generation depends on the whole translation unit.
#pragma once
#include "grape_walk_core.hpp"
#include "grape_walk_gauge.hpp"

namespace grape {

// ---------------------------------------------------------------------------
// Merged phase-covariant walks (round 5): BOTH sector classes of the Rydberg layout in one lane
// ---------------------------------------------------------------------------
// The C2 walks are VALU-issue bound (≈ 84 % of SIMD cycles issue VALU instructions in every one of
// the four walk kernels, profiles/r05/final_c2 instruction mix), and the two classes' lanes of one
// (evaluation, chunk) repeat the same per-step work: the load of x_k, e^{i a x_k}, e^{i phi} - 1,
// the loop.  A merged lane walks class A (one sector of DA levels) and class B (two 2-level
// sectors, twins or not) over the same chunk, sharing that work, and its gradient walk writes ONE
// F_dx part, part_A + part_B -- the value k_sec_reduce would have formed from the two parts in either class
// order -- so the reduction reads one part.  Per class the operations are the
// gauge walks' own (walk_fwd_body / walk_grad_body with GAUGE) but for the step phase e^{i a x_k}, which
// the merged kernels take from a table in LDS (gauge_cis_tab): at equal chunking the results are those of
// the per-class kernels to rounding.  Both classes take class A's chunking (the engine
// sets class B's L and nchunks to class A's).
// E~ of the merged walks (round 6; SMEM of gauge_prop_lds): from the plan's global copy
// (DevProblem::gauge_Et) through scalar loads -- E~ is launch-uniform, so each entry is an SGPR operand of the
// complex product that forms E_k -- re-issued every step (the pointer is made opaque per step, so the loads are
// not hoisted into 13 complex registers held across the walk).  The forward walks, the rank-one gradient walk
// (merged_step_grad_r1) and the wide pass take E~ this way; the matrix gradient walk (merged_step_grad) keeps
// E~ from LDS (gauge_base_lds) in registers at two waves, where the per-step scalar loads sat on its critical
// path.
template <int D, bool SMEM>
__device__ __forceinline__ void gauge_prop_lds(const cd *Et, const cd (&e)[kGaugePairs<D>],
                                               MStore<D, false> &E) {  // gauge_prop, E~ in LDS or (SMEM) global
    if constexpr (SMEM) {
        cptr<cd> g = as_constant(Et);
        asm volatile("" : "+s"(g));
#pragma unroll
        for (int j = 0; j < D; ++j) {
#pragma unroll
            for (int k = 0; k < D; ++k) E.set(j, k, gauge_sandwich<D>(e, j, k, cload(g, j * D + k)));
        }
    } else {
#pragma unroll
        for (int j = 0; j < D; ++j) {
#pragma unroll
            for (int k = 0; k < D; ++k) E.set(j, k, gauge_sandwich<D>(e, j, k, Et[j * D + k]));
        }
    }
}
// E~ = exp(-i dt H_w(0)) of sectors w < nsec of a class into out [nsec][D][D] row-major: gauge_base_lds's
// code (the nominal build at x = 0, the walks' exponential, unshifted), one lane per sector
template <int D>
__global__ __launch_bounds__(64) void k_gauge_base_fill(DevProblem P, cd *scr, cd *out, int nsec) {
    const int w = threadIdx.x;
    if (w >= nsec) return;
    WalkX X0;
    X0.k0 = X0.k1 = X0.a0 = X0.a1 = 0.0;
    Pert none;
    none.var = -1;
    none.index = 0;
    none.delta = 0.0;
    SM<D> A[1];
    walk_build<D, 1>(P, as_constant(P.ops) + (size_t)w * P.sec_ops, X0, 1, none, A);
    double mu0 = 0.0;
    walk_expm<D, false, false>(A[0], scr + (size_t)w * 2 * D * D, mu0, true, [&](int i, const cd (&x)[D]) {
#pragma unroll
        for (int j = 0; j < D; ++j) out[(w * D + j) * D + i] = x[j];
    });
}
template <int D, int NE, bool LAD>
__device__ __forceinline__ void merged_step_fwd(const cd *Et, const GaugeN<D> (&gn)[NE], cd p1, cd (&Q)[NE][D][D]) {
#pragma unroll
    for (int w = 0; w < NE; ++w) {
        cd dph[kGaugePairs<D>];
        if constexpr (LAD) gauge_phases_ladder<D>(p1, dph);
        else gauge_phases<D>(p1, gn[w], dph);
        MStore<D, false> E;
        gauge_prop_lds<D, true>(Et + w * D * D, dph, E);
#pragma unroll
        for (int i = 0; i < D; ++i) {  // column i of E_k Q (the forward walk's order)
            cd q[D], t[D];
#pragma unroll
            for (int m = 0; m < D; ++m) q[m] = Q[w][m][i];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                cd c = czero();
#pragma unroll
                for (int m = 0; m < D; ++m) cmac(c, q[m], E.at(j, m));
                t[j] = c;
            }
#pragma unroll
            for (int j = 0; j < D; ++j) Q[w][j][i] = t[j];
        }
    }
}
// ---------------------------------------------------------------------------
// The wide pass (round 8): one lane per evaluation over all N_t steps, no time chunks
// ---------------------------------------------------------------------------
// The chunk totals, the carries and k_scan_seq exist because time is cut into chunks to fill the GPU at
// max_batch evaluations per pass.  A device-resident call of at least W = max_batch x nchunks evaluations
// fills the same lanes with one evaluation each, and a rank-one plan (DevProblem::rank1) then needs no S x S
// chain at all: the diagonal head reads only U_cc of each sector and writes m = alpha U_c. (row c of M), so
//   psi_N = U e_c (one vector, walked forward from e_c),   phi_N = conj(alpha) e_c (no walk),
// and the gradient walk runs time-reversed from them, psi_{k-1} = E_k^dag psi_k (E_k = D_k E~ D_k^dag is
// unitary: Hermitian H0), phi_{k-1} = E_k^dag phi_k, contracting conj(phi_k,r) (E_k)_rj psi_{k-1},j at every
// step -- the chunked rank-one walk's quantity at the chunked walk's instruction count, 9 + 4 complex MACs per
// forward step where the chain takes 27 + 4.  The recomputed psi_{k-1} carries the non-unitarity of the
// computed E_k, about one rounding per step: the engine takes the wide pass up to N_t = 4096 only.
// One launch per stage; the lane's chunk is the whole pulse (P.nchunks = 1, P.L = N_t in the launch's copies).
struct WideLane {
    int be, nbe;
    bool ok;
};
__device__ __forceinline__ WideLane wide_lane(const DevBatch &BA) {  // (class A: one sector, BA.nb evaluations)
    WideLane L;
    const long g = (long)blockIdx.x * kWalkBlock + threadIdx.x;
    L.nbe = BA.nb;
    L.ok = g < (long)L.nbe;
    L.be = L.ok ? (int)g : 0;  // lanes past the end walk evaluation 0 and store nothing
    return L;
}
// psi <- E_k psi over NE propagators (merged_step_fwd's E formation, E~ through scalar loads)
template <int D, int NE, bool LAD>
__device__ __forceinline__ void wide_step_fwd(const cd *Et, const GaugeN<D> (&gn)[NE], cd p1, cd (&psi)[NE][D]) {
#pragma unroll
    for (int w = 0; w < NE; ++w) {
        cd dph[kGaugePairs<D>];
        if constexpr (LAD) gauge_phases_ladder<D>(p1, dph);
        else gauge_phases<D>(p1, gn[w], dph);
        MStore<D, false> E;
        gauge_prop_lds<D, true>(Et + w * D * D, dph, E);
        cd t[D];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            cd c = czero();
#pragma unroll
            for (int m = 0; m < D; ++m) cmac(c, psi[w][m], E.at(j, m));
            t[j] = c;
        }
#pragma unroll
        for (int j = 0; j < D; ++j) psi[w][j] = t[j];
    }
}
// The forward walk in the step frame (ladder charges).  With D_k = diag(p_k^j) (gauge_phases_ladder: e_jm =
// conj(p^(m-j)), so E_jm = p^j E~_jm p^-m and level j carries charge j), chi_k = D_k^dag psi_k obeys
//   chi_k = E~ diag(dl^j) chi_{k-1},   dl = p_{k-1} conj(p_k) = e^{i a (x_{k-1} - x_k)}   (x before the first step: 0)
// so a step never forms E_k: the re-framing takes dl, dl^2 and D - 1 complex products per sector (16 VALU
// instructions for one 3-level and one 2-level chain where E_k's formation takes 36), and E~'s entries are the
// scalar operands of the 9 + 4 complex MACs themselves.  dl is the table phase of the controls' difference: one
// subtraction where the product of two phases takes four instructions and a carried phase two registers, and its
// argument is rounded as a x_k is.  psi_N = D_{N-1} chi_N: one closing re-framing by the last step's phase.  The
// same quantity as wide_step_fwd, other roundings.
template <int D, int NE, int DP>
__device__ __forceinline__ void wide_reframe(const cd (&pw)[DP], cd (&chi)[NE][D]) {  // chi_j <- pw[j] chi_j, pw[0] = 1
    static_assert(D <= DP, "powers up to the sector's highest charge");
#pragma unroll
    for (int w = 0; w < NE; ++w) {
#pragma unroll
        for (int j = 1; j < D; ++j) chi[w][j] = cmulf(chi[w][j], pw[j]);
    }
}
template <int D, int NE>
__device__ __forceinline__ void wide_step_frame(const cd *Et, cd (&chi)[NE][D]) {  // chi <- E~ chi
#pragma unroll
    for (int w = 0; w < NE; ++w) {
        cptr<cd> g = as_constant(Et + w * D * D);  // (per-step scalar loads, as gauge_prop_lds<D, true>)
        asm volatile("" : "+s"(g));
        cd t[D];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            cd c = czero();
#pragma unroll
            for (int m = 0; m < D; ++m) cmac(c, chi[w][m], cload(g, j * D + m));
            t[j] = c;
        }
#pragma unroll
        for (int j = 0; j < D; ++j) chi[w][j] = t[j];
    }
}
// psi_N of one chain for the head (k_wide_head reads entry c: U_cc) and the gradient walk's start, evaluation-minor:
// entry j at u[j * nbe] (u: the chain's first entry of this evaluation), so a wave's stores and loads are contiguous
template <int D>
__device__ __forceinline__ void wide_store_psi(cd *u, size_t nbe, const cd (&psi)[D]) {
#pragma unroll
    for (int j = 0; j < D; ++j) u[j * nbe] = psi[j];
}
// The controls of the workgroup's kWalkBlock evaluations over one tile of kFdxTile steps, [row][step] in LDS:
// sixteen lanes read one row's 128-byte piece per instruction, so every line of x is fetched once and used
// whole.  (A lane streaming its own row touches one line per lane and step and finds it evicted eight steps
// later at 262 144 lanes: the first cut of the wide walks fetched 4.8 GB per forward launch for 1.08 GB of
// controls.)  The tile is loaded where it is needed: the load itself is cheap (cutting the tile
// blocks moved nothing), but a wave spends a sixth to a quarter of its life between the end of a tile's steps and
// the barrier behind the next load, waiting for its workgroup's other wave, which sits on another SIMD at another
// place of that SIMD's queue (profiles/r15/attribution.txt; wide_set_prio keeps the waves of a SIMD together),
// and a register copy of the next tile (16 values and their addresses per lane) cost the
// gradient walk its fourth wave.  Rows past the last evaluation read the last one's.
constexpr int kFdxTile = 16;  // steps per tile: the wide walks' x tiles, the merged gradient walks' F_dx flush
__device__ __forceinline__ void wide_load_x(double (*tile)[kFdxTile + 1], const double *x, int nx, int nbe, int j0, int Nt) {
    constexpr int kStep = kWalkBlock / kFdxTile;  // rows per instruction
    const int j = threadIdx.x % kFdxTile, r0 = threadIdx.x / kFdxTile;
    const double *xc = x + min(j0 + j, Nt - 1);
    const long b0 = (long)blockIdx.x * kWalkBlock;
#pragma unroll 4
    for (int r = r0; r < kWalkBlock; r += kStep) tile[r][j] = xc[(size_t)min(b0 + r, (long)nbe - 1) * nx];
}
// The same tile, and the gradient walk's F_dx flush, where nothing needs a clamp or a predicate: every row of the
// workgroup is an evaluation (wide_group_full) and every slot of the tile a step (j0 + kFdxTile <= N_t).  Row
// r0 + 8 i, slot j of the workgroup's tile is element (8 i nx) + (r0 nx + j) of the workgroup's first row at j0:
// a uniform base stepped by a uniform stride, plus one per-lane offset (wide_tile_offset) formed once per kernel
// -- one address add per element, where wide_load_x spends 11 VALU instructions per load and the predicated
// flush 16 per store -- and the LDS addresses are immediates.  The same elements to and from the same slots.
__device__ __forceinline__ bool wide_group_full(int nbe) {
    return GRAPE_WIDE_TILE_FAST && ((long)blockIdx.x + 1) * kWalkBlock <= (long)nbe;
}
__device__ __forceinline__ unsigned wide_tile_offset(int nx) {
    // in bytes, 32 bits: r0 < kWalkBlock / kFdxTile = 8 rows of nx <= 4097 doubles (the wide pass stops at
    // N_t = 4096: wide_ok) and j < 16 make it at most 8 (7 x 4097 + 15) < 2^18
    return (unsigned)((threadIdx.x / kFdxTile) * nx + threadIdx.x % kFdxTile) * (unsigned)sizeof(double);
}
__device__ __forceinline__ void wide_load_x_full(double (*tile)[kFdxTile + 1], const double *xb, int nx, unsigned off) {
    constexpr int kStep = kWalkBlock / kFdxTile, kTrips = kWalkBlock / kStep;
    const int j = threadIdx.x % kFdxTile, r0 = threadIdx.x / kFdxTile;
    double v[kTrips];
#pragma unroll
    for (int i = 0; i < kTrips; ++i)
        v[i] = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(xb + (size_t)i * kStep * nx) + off);
#pragma unroll
    for (int i = 0; i < kTrips; ++i) tile[r0 + i * kStep][j] = v[i];
}
__device__ __forceinline__ void wide_flush_full(const double (*tile)[kFdxTile + 1], double *fb, int nx, unsigned off) {
    constexpr int kStep = kWalkBlock / kFdxTile, kTrips = kWalkBlock / kStep;
    const int j = threadIdx.x % kFdxTile, r0 = threadIdx.x / kFdxTile;
#pragma unroll
    for (int i = 0; i < kTrips; ++i)
        *reinterpret_cast<double *>(reinterpret_cast<char *>(fb + (size_t)i * kStep * nx) + off) = tile[r0 + i * kStep][j];
}
// In-kernel stamps of the wide walks -- a diagnostic build only (-DGRAPE_WIDE_STAMPS=1 through
// scripts/build_variants.py; scripts/probes/wide_attribution.py reads them): the default build defines nothing of
// this and WideStamp is empty.  Every wave takes the shader clock (s_memtime) and the constant 100 MHz clock
// (s_memrealtime) before its first tile and after its last, sums the shader clocks it spent in tile seams (from the
// end of a tile's steps, or the start, to the barrier behind the next tile's load), and its first lane writes them
// with where the wave ran (HW_ID, XCC_ID) to a buffer no kernel reads.
#ifdef GRAPE_WIDE_STAMPS
constexpr int kWideStampWaves = 8192, kWideStampWords = 8;
static __device__ unsigned long long g_wide_stamps[2][kWideStampWaves][kWideStampWords];
struct WideStamp {
    unsigned long long t0, r0, ts, seam;
    unsigned nseam;
    __device__ __forceinline__ void begin() {
        t0 = ts = __builtin_amdgcn_s_memtime();
        r0 = __builtin_amdgcn_s_memrealtime();
        seam = 0;
        nseam = 0;
    }
    __device__ __forceinline__ void seam_in() { ts = __builtin_amdgcn_s_memtime(); }
    __device__ __forceinline__ void seam_out() {
        seam += __builtin_amdgcn_s_memtime() - ts;
        ++nseam;
    }
    __device__ __forceinline__ void end(int kernel) {
        const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        const unsigned hw = __builtin_amdgcn_s_getreg(4 | (31 << 11)), xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));
        const unsigned wave = blockIdx.x * (kWalkBlock / 64) + threadIdx.x / 64;
        if (threadIdx.x % 64 == 0 && wave < (unsigned)kWideStampWaves) {
            unsigned long long *o = g_wide_stamps[kernel][wave];
            o[0] = t0, o[1] = r0, o[2] = t1, o[3] = r1, o[4] = seam, o[5] = ((unsigned long long)xcc << 32) | hw;
            o[6] = nseam, o[7] = 1;
        }
    }
};
#else
struct WideStamp {
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void seam_in() {}
    __device__ __forceinline__ void seam_out() {}
    __device__ __forceinline__ void end(int) {}
};
#endif
// A wave's issue priority from its own progress.  The four waves of a SIMD start together (one round of workgroups
// fills the chip at 262 144 lanes) and VALU issue goes by priority, then age: left alone, the oldest wave runs
// nearly unimpeded and the four finish one after another -- at 0.47, 0.57, 0.82 and 0.94 of the kernel, the last
// alone for a ninth of it, and even the wave that finishes first issues in under half the cycles of its life
// (profiles/r15/attribution.txt).  So a wave
// sets its priority once per tile from the quarter of the walk it is in, 3, 2, 1, 0: a wave that is behind outranks
// one that is ahead, the spread is held within a quarter of the walk (a wave that crosses into the next quarter
// yields to every wave still in this one), and only the last quarter drains in age order.  With it the waves
// finished at 0.81 .. 0.96 (stamps of a tree whose forward walk also had a per-tile guard, since taken out: DESIGN.md
// 9).  s_setprio is scalar and ignores EXEC: it sits where the whole wave passes once per tile.
// (Two tiles a level, cyclic, closed the finish times less -- a wave that wraps outranks the ones it left behind --
// and measured 154 M evaluations/s where this measured 157, both on that tree: DESIGN.md 9.)
// Measured at the one shape where all waves of a SIMD start together: C2, one round of workgroups.  With more
// than one round a fresh wave at priority 3 outranks resident waves near their end, which that measurement does not
// cover; a walk of fewer than four tiles never reaches the last quarter, so the walks put the priority back to 0
// behind their last tile (wide_reset_prio) and no epilogue runs above it.
__device__ __forceinline__ void wide_set_prio(int done, int of) {  // done of `of` tiles walked (wave-uniform)
    const int d4 = 4 * done;  // the quarter is floor(4 done / of), by compares: no scalar division
    if (d4 < of) __builtin_amdgcn_s_setprio(3);
    else if (d4 < 2 * of) __builtin_amdgcn_s_setprio(2);
    else if (d4 < 3 * of) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}
__device__ __forceinline__ void wide_reset_prio() { __builtin_amdgcn_s_setprio(0); }
template <int DA, bool TWB, bool LAD>
__device__ __forceinline__ void wide_fwd_body(const DevProblem &PA, const DevBatch &BA, const DevProblem &PB,
                                              const DevBatch &BB) {
    constexpr int NEB = TWB ? 1 : 2;
    __shared__ double xtile[kWalkBlock][kFdxTile + 1];  // (+1: conflict-free rows)
    __shared__ grape_cis::CisTabEntry ctab[grape_cis::kCisTabN];
    gauge_cis_stage(ctab);
    const WideLane L = wide_lane(BA);
    GaugeN<DA> gA[1];
    GaugeN<2> gB[NEB];
    gA[0] = gauge_charges<DA>(PA, 0);
#pragma unroll
    for (int w = 0; w < NEB; ++w) gB[w] = gauge_charges<2>(PB, w);
    const int cA = PA.rank1_c[0];
    cd psiA[1][DA], psiB[NEB][2];
#pragma unroll
    for (int j = 0; j < DA; ++j) psiA[0][j] = cmake(j == cA ? 1.0 : 0.0, 0.0);
#pragma unroll
    for (int w = 0; w < NEB; ++w) {
#pragma unroll
        for (int j = 0; j < 2; ++j) psiB[w][j] = cmake(j == PB.rank1_c[w] ? 1.0 : 0.0, 0.0);
    }
    constexpr bool FRAME = LAD && GRAPE_WIDE_STEP_FRAME;  // (psi holds chi = D_k^dag psi: wide_step_frame)
    double xprev = 0.0;  // (the control of the step before: dl from the difference, the first dl conj(p_0))
    auto step = [&](double xk) {
        if constexpr (FRAME) {
            cd pw[DA];
            ladder_powers<DA>(gauge_cis_tab(PA.gauge_a * (xprev - xk), ctab), pw);
            xprev = xk;
            wide_reframe<DA, 1>(pw, psiA);
            wide_reframe<2, NEB>(pw, psiB);
            wide_step_frame<DA, 1>(PA.gauge_Et, psiA);
            wide_step_frame<2, NEB>(PB.gauge_Et, psiB);
        } else {
            const cd p1 = gauge_cis_tab(PA.gauge_a * xk, ctab);
            wide_step_fwd<DA, 1, LAD>(PA.gauge_Et, gA, p1, psiA);
            wide_step_fwd<2, NEB, LAD>(PB.gauge_Et, gB, p1, psiB);
        }
    };
    const bool full = wide_group_full(L.nbe);
    const unsigned off = wide_tile_offset(PA.nx);
    const double *xb = BA.x + (size_t)blockIdx.x * kWalkBlock * PA.nx;  // the workgroup's first row
    WideStamp stamp;  // (empty but in the diagnostic build)
    stamp.begin();
#pragma unroll 1
    for (int j0 = 0; j0 < PA.Nt; j0 += kFdxTile) {
        const int nj = min(kFdxTile, PA.Nt - j0);
        wide_set_prio(j0 / kFdxTile, (PA.Nt + kFdxTile - 1) / kFdxTile);
        if (full && j0 + kFdxTile <= PA.Nt) wide_load_x_full(xtile, xb + j0, PA.nx, off);
        else wide_load_x(xtile, BA.x, PA.nx, L.nbe, j0, PA.Nt);
        __syncthreads();
        stamp.seam_out();
        int t = 0;  // (unrolled by hand, as k_walk_fwd_m below)
#pragma unroll 1
        for (; t + 1 < nj; t += 2) {
            step(xtile[threadIdx.x][t]);
            step(xtile[threadIdx.x][t + 1]);
        }
        if (t < nj) step(xtile[threadIdx.x][t]);
        stamp.seam_in();
        __syncthreads();
    }
    wide_reset_prio();
    stamp.end(0);
    if constexpr (FRAME) {  // psi_N = D_{N-1} chi_N: the head and the gradient walk read the lab frame
        cd pw[DA];
        ladder_powers<DA>(gauge_cis_tab(PA.gauge_a * xprev, ctab), pw);  // (the last step's phase, once per kernel)
        wide_reframe<DA, 1>(pw, psiA);
        wide_reframe<2, NEB>(pw, psiB);
    }
    if (L.ok) {
        wide_store_psi<DA>(BA.Ub + L.be, (size_t)L.nbe, psiA[0]);
#pragma unroll
        for (int w = 0; w < NEB; ++w)  // (twins: one chain serves both sectors)
            wide_store_psi<2>(BB.Ub + (size_t)w * 2 * L.nbe + L.be, (size_t)L.nbe, psiB[w]);
    }
}
template <int DA, bool TWB, bool LAD, bool WIDE = false>
__global__ __launch_bounds__(kWalkBlock, (WIDE ? GRAPE_WALK_WIDE_FWD_WAVES : GRAPE_WALK_FWD_M_WAVES)) void k_walk_fwd_m(DevProblem PA, DevBatch BA,
                                                                                  DevProblem PB, DevBatch BB) {
    if constexpr (WIDE) {
        wide_fwd_body<DA, TWB, LAD>(PA, BA, PB, BB);
        return;
    }
    constexpr int NEB = TWB ? 1 : 2;
    __shared__ grape_cis::CisTabEntry ctab[grape_cis::kCisTabN];
    gauge_cis_stage(ctab);
    const VBlock vb = hw_block();
    const WalkLane L = walk_lane<1>(PA, BA, vb);  // (class A: one sector; its chunking is both classes')
    const double *xt = BA.x + (size_t)L.be * PA.nx;  // this evaluation's row of x
    const cd *EtA = PA.gauge_Et, *EtB = PB.gauge_Et;  // (through scalar loads: gauge_prop_lds)
    GaugeN<DA> gA[1];
    GaugeN<2> gB[NEB];
    gA[0] = gauge_charges<DA>(PA, 0);
#pragma unroll
    for (int w = 0; w < NEB; ++w) gB[w] = gauge_charges<2>(PB, w);
    cd QA[1][DA][DA], QB[NEB][2][2];
#pragma unroll
    for (int j = 0; j < DA; ++j) {
#pragma unroll
        for (int i = 0; i < DA; ++i) QA[0][j][i] = cmake(i == j ? 1.0 : 0.0, 0.0);
    }
#pragma unroll
    for (int w = 0; w < NEB; ++w) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) QB[w][j][i] = cmake(i == j ? 1.0 : 0.0, 0.0);
        }
    }
    const int k0 = L.c * PA.L;
    X2 xn = walk_load_x(1, xt + (size_t)min(k0, PA.Nt - 1));
    auto step = [&](int jj) {
        const int k = min(k0 + jj, PA.Nt - 1);
        const double xk = xn.v0;
        xn = walk_load_x(1, xt + (size_t)min(k + 1, PA.Nt - 1));  // next step's control
        const cd p1 = gauge_cis_tab(PA.gauge_a * xk, ctab);  // e^{i a x_k}, both classes (the engine checks one a)
        merged_step_fwd<DA, 1, LAD>(EtA, gA, p1, QA);
        merged_step_fwd<2, NEB, LAD>(EtB, gB, p1, QB);
    };
    // steps past N_t leave Q alone: only the last chunk has them, so the first n_last steps of every
    // chunk run unpredicated and the rest only in the other chunks' lanes (a branch, not selects)
    const int nlast = PA.Nt - (PA.nchunks - 1) * PA.L;
    // unrolled by hand (two steps per trip, then the odd one: no loop-carried register moves): the phases'
    // constants pass through an inline asm (gauge_cis_tab), which LLVM treats as convergent and will not runtime-unroll
    int j2 = 0;
#pragma unroll 1
    for (; j2 + 1 < nlast; j2 += 2) {
        step(j2);
        step(j2 + 1);
    }
#pragma unroll 1
    for (; j2 < nlast; ++j2) step(j2);
#pragma unroll 1
    for (int jj = nlast; jj < PA.L; ++jj) {
        if (L.c != PA.nchunks - 1) step(jj);
    }
    if (L.ok) {  // chunk totals lane-minor (k_scan_seq's coalesced reads): [c][element][evaluation]
        const size_t nbe = (size_t)L.nbe;
        cd *da = BA.Tc + (size_t)L.c * DA * DA * nbe + L.be;
#pragma unroll
        for (int j = 0; j < DA; ++j) {
#pragma unroll
            for (int i = 0; i < DA; ++i) da[(size_t)(j * DA + i) * nbe] = QA[0][j][i];
        }
#pragma unroll
        for (int w = 0; w < NEB; ++w) {  // (twins: one chain)
            cd *db = BB.Tc + ((size_t)w * PB.nchunks + L.c) * 4 * nbe + L.be;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int i = 0; i < 2; ++i) db[(size_t)(j * 2 + i) * nbe] = QB[w][j][i];
            }
        }
    }
}
// The merged path's scan: one lane per evaluation walks its chunk totals in order,
// Carry_0 = I, Carry_{c+1} = T_c Carry_c, U = T_{n-1} Carry_{n-1} -- 2 x (n - 1) small products per
// lane where k_scan_pair spends a wave per sub-evaluation on a Hillis-Steele scan, and every read and
// carry write coalesced (lane-minor [c][element][evaluation]); U row-major per sub-evaluation, as
// the sector head reads it.  (The association of the chain differs from k_scan's: rounding only.)
// Round 5: both classes' chains advance in one loop over the chunks (class B has class A's chunk
// count on merged passes), each with its next chunk total in flight while the current product runs,
// in one-wave workgroups (32 768 evaluations: 2 waves on every CU): 0.064 -> 0.057 ms per C2 pass.
// The pass moves ~26 tiles per (evaluation, chunk) through HBM, so the scan runs near the HBM rate;
// three column lanes per evaluation (more waves, same bytes) measured 0.059 ms.
template <int D>
struct SeqChain {
    const cd *T;
    cd *Carry;
    cd P[D][D], tn[D][D];
    __device__ __forceinline__ void init(const cd *T_, cd *Carry_, size_t nbe, size_t be) {
        T = T_ + be;
        Carry = Carry_ + be;
#pragma unroll
        for (int e = 0; e < D * D; ++e) {
            P[e / D][e % D] = cmake(e / D == e % D ? 1.0 : 0.0, 0.0);
            tn[e / D][e % D] = T[(size_t)e * nbe];
        }
    }
    __device__ __forceinline__ void step(int c, int nch, size_t nbe) {
        cd *dc = Carry + (size_t)c * D * D * nbe;
        const cd *tc = T + (size_t)min(c + 1, nch - 1) * D * D * nbe;
        cd t[D][D];
#pragma unroll
        for (int j = 0; j < D; ++j) {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                dc[(size_t)(j * D + i) * nbe] = P[j][i];
                t[j][i] = tn[j][i];
                tn[j][i] = tc[(size_t)(j * D + i) * nbe];
            }
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {  // P <- T_c P, column by column
            cd q[D];
#pragma unroll
            for (int m = 0; m < D; ++m) q[m] = P[m][i];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                cd acc = czero();
#pragma unroll
                for (int m = 0; m < D; ++m) cmac(acc, t[j][m], q[m]);
                P[j][i] = acc;
            }
        }
    }
};
constexpr int kSeqBlock = 64;
template <int DA, bool TWB>
__global__ __launch_bounds__(kSeqBlock) void k_scan_seq(DevProblem PA, DevBatch BA, DevProblem PB, DevBatch BB, int nb) {
    constexpr int NEB = TWB ? 1 : 2;
    const size_t be = (size_t)blockIdx.x * kSeqBlock + threadIdx.x;
    if (be >= (size_t)nb) return;
    const size_t nbe = (size_t)nb;
    const int nch = PA.nchunks;  // (== PB.nchunks: the engine gives class B class A's chunking)
    SeqChain<DA> ca;
    SeqChain<2> cb[NEB];
    ca.init(BA.Tc, BA.Carry, nbe, be);
#pragma unroll
    for (int w = 0; w < NEB; ++w)
        cb[w].init(BB.Tc + (size_t)w * PB.nchunks * 4 * nbe, BB.Carry + (size_t)w * PB.nchunks * 4 * nbe, nbe, be);
#pragma unroll 1
    for (int c = 0; c < nch; ++c) {
        ca.step(c, nch, nbe);
#pragma unroll
        for (int w = 0; w < NEB; ++w) cb[w].step(c, nch, nbe);
    }
    cd *ua = BA.Ub + be * DA * DA;
#pragma unroll
    for (int j = 0; j < DA; ++j) {
#pragma unroll
        for (int i = 0; i < DA; ++i) ua[j * DA + i] = ca.P[j][i];
    }
#pragma unroll
    for (int w = 0; w < NEB; ++w) {
#pragma unroll
        for (int ws = 0; ws < (TWB ? 2 : 1); ++ws) {  // (twins: both sectors' U)
            cd *ub = BB.Ub + (be * 2 + w + ws) * 4;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int i = 0; i < 2; ++i) ub[j * 2 + i] = cb[w].P[j][i];
            }
        }
    }
}
// one gradient step of NSEC sectors over NE propagators (NSH = NSEC / NE sectors share one):
// Y = X E^dag, the contraction, X <- E Y; returns the sectors' terms summed in sector order
// ((0 + s_0) + s_1 ...; one sector: s_0)
template <int D, int NE, int NSEC, bool LAD>
__device__ __forceinline__ double merged_step_grad(const cd *Et, const GaugeN<D> (&gn)[NE], cd p1, cd q,
                                                   double inv_eps, cd (&X)[NSEC][D][D]) {
    constexpr int NSH = NSEC / NE;
    MStore<D, false> E[NE];
#pragma unroll
    for (int w = 0; w < NE; ++w) {
        cd dph[kGaugePairs<D>];
        if constexpr (LAD) gauge_phases_ladder<D>(p1, dph);
        else gauge_phases<D>(p1, gn[w], dph);
        gauge_prop_lds<D, false>(Et + w * D * D, dph, E[w]);
    }
#pragma unroll
    for (int w = 0; w < NSEC; ++w) {  // Y = X E^dag, row by row
        const int we = w / NSH;
#pragma unroll
        for (int r = 0; r < D; ++r) {
            cd xr[D], y[D];
#pragma unroll
            for (int j = 0; j < D; ++j) xr[j] = X[w][r][j];
#pragma unroll
            for (int cc = 0; cc < D; ++cc) {
                cd s = czero();
#pragma unroll
                for (int j = 0; j < D; ++j) cmac(s, xr[j], cconj(E[we].at(cc, j)));
                y[cc] = s;
            }
#pragma unroll
            for (int cc = 0; cc < D; ++cc) X[w][r][cc] = y[cc];
        }
    }
    double tot = 0.0, one = 0.0;
    if constexpr (LAD && GRAPE_WALK_LADDER_CONTR) {
        // Ladder charges: f_rj = rho(r - j) for r > j and conj(rho(j - r)) for r < j, so with
        // T_m = sum_{r - j = m} Y_jr E_rj + conj(sum_{r - j = -m} Y_jr E_rj) (m = 1 .. D-1)
        //   sum_{r != j} Re(Y_jr E_rj f_rj) = sum_m Re(rho(m) T_m):
        // one complex MAC per off-diagonal entry and one product per charge difference, where the
        // per-entry form spends E_rj f_rj / eps and a real MAC pair on every entry (same quantity,
        // other roundings)
        cd rh[D];
        ladder_rho<D>(q, rh);
#pragma unroll
        for (int we = 0; we < NE; ++we) {
#pragma unroll
            for (int t = 0; t < NSH; ++t) {
                double tre[D], tim[D];
#pragma unroll
                for (int m = 0; m < D; ++m) tre[m] = tim[m] = 0.0;
#pragma unroll
                for (int r = 0; r < D; ++r) {
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        if (r == j) continue;
                        const int m = r > j ? r - j : j - r;
                        const cd y = X[we * NSH + t][j][r], e = E[we].at(r, j);
                        tre[m] = fma(y.re, e.re, tre[m]);
                        tre[m] = fma(-y.im, e.im, tre[m]);
                        if (r > j) {
                            tim[m] = fma(y.re, e.im, tim[m]);
                            tim[m] = fma(y.im, e.re, tim[m]);
                        } else {
                            tim[m] = fma(-y.re, e.im, tim[m]);
                            tim[m] = fma(-y.im, e.re, tim[m]);
                        }
                    }
                }
                double c = 0.0;
#pragma unroll
                for (int m = 1; m < D; ++m) {
                    c = fma(rh[m].re, tre[m], c);
                    c = fma(-rh[m].im, tim[m], c);
                }
                const double sv = c * inv_eps;
                tot += sv;
                one = sv;
            }
        }
    } else {
#pragma unroll
    for (int we = 0; we < NE; ++we) {
        double s[NSH];
#pragma unroll
        for (int t = 0; t < NSH; ++t) s[t] = 0.0;
        cd fw[kGaugePairs<D>];
        gauge_fd_weights_dn<D>(q, gn[we], fw);
#pragma unroll
        for (int r = 0; r < D; ++r) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                if (r == j) continue;
                const cd de = cscale(inv_eps, cmul(E[we].at(r, j), gauge_fd_weight<D>(fw, r, j)));
#pragma unroll
                for (int t = 0; t < NSH; ++t) {
                    const cd y = X[we * NSH + t][j][r];
                    s[t] = fma(y.re, de.re, s[t]);
                    s[t] = fma(-y.im, de.im, s[t]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NSH; ++t) {
            tot += s[t];
            one = s[t];
        }
    }
    }
#pragma unroll
    for (int w = 0; w < NSEC; ++w) {  // X <- E Y, column by column
        const int we = w / NSH;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            cd y[D], t[D];
#pragma unroll
            for (int m = 0; m < D; ++m) y[m] = X[w][m][i];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                cd c = czero();
#pragma unroll
                for (int m = 0; m < D; ++m) cmac(c, E[we].at(j, m), y[m]);
                t[j] = c;
            }
#pragma unroll
            for (int j = 0; j < D; ++j) X[w][j][i] = t[j];
        }
    }
    return NSEC > 1 ? tot : one;
}
// The rank-one gradient step (R1, DevProblem::rank1).  With the diagonal head every sector's M block has
// one non-zero row, M = e_c m^T (grape_projector.hip diag_row: row r carries the factor W[g_r]), so
//   X_k = Q_k M Q_k^dag = psi_k phi_k^dag,   psi_k = Q_k e_c,   phi_k = Q_k conj(m)
// for the whole walk, and the matrix step's Y = X E^dag, X <- E Y are two matrix-vector products:
//   phi <- E_k phi;   Y_jr = psi_j conj(phi_r);   psi <- E_k psi
// -- the same quantity, no approximation.  The products u_rj = E_rj psi_j are taken once and serve both the
// contraction (T_m from conj(phi_r) u_rj, grouped by charge difference as above) and psi <- sum_j u_rj.
// Per 3-level sector and step: 36 FMA (phi) + 18 MUL + 18 FMA (u) + 24 FMA (T) + 12 ADD (psi), where the
// matrix step spends 216 FMA on its two products and 24 on the contraction.
// Its registers (24 VGPRs of state where the matrix walk holds 36, no Y) leave room for a third wave per SIMD once
// E~ comes through scalar loads (108 VGPRs, no scratch; with E~ from LDS in registers the
// lane spills at three waves), and there the scalar loads pay.  The matrix walk keeps
// GRAPE_WALK_MERGED_WAVES and E~ from LDS.
template <int D, int NE, int NSEC, bool LAD>
__device__ __forceinline__ double merged_step_grad_r1(const cd *Et, const GaugeN<D> (&gn)[NE], cd p1, cd q,
                                                      double inv_eps, cd (&psi)[NSEC][D], cd (&phi)[NSEC][D]) {
    constexpr int NSH = NSEC / NE;
    MStore<D, false> E[NE];
#pragma unroll
    for (int w = 0; w < NE; ++w) {
        cd dph[kGaugePairs<D>];
        if constexpr (LAD) gauge_phases_ladder<D>(p1, dph);
        else gauge_phases<D>(p1, gn[w], dph);
        gauge_prop_lds<D, true>(Et + w * D * D, dph, E[w]);
    }
    cd rh[D];
    if constexpr (LAD) ladder_rho<D>(q, rh);
    double tot = 0.0, one = 0.0;
#pragma unroll
    for (int we = 0; we < NE; ++we) {
        cd fw[kGaugePairs<D>];
        if constexpr (!LAD) {
            gauge_fd_weights_dn<D>(q, gn[we], fw);
        }
#pragma unroll
        for (int t = 0; t < NSH; ++t) {
            const int w = we * NSH + t;
            cd f[D], u[D][D];
#pragma unroll
            for (int r = 0; r < D; ++r) {  // phi <- E phi
                cd c = czero();
#pragma unroll
                for (int j = 0; j < D; ++j) cmac(c, E[we].at(r, j), phi[w][j]);
                f[r] = c;
            }
#pragma unroll
            for (int r = 0; r < D; ++r) {
                phi[w][r] = f[r];
#pragma unroll
                for (int j = 0; j < D; ++j) u[r][j] = cmulf(E[we].at(r, j), psi[w][j]);
            }
            double c = 0.0;
            if constexpr (LAD) {  // T_m = sum_{r-j=m} conj(phi_r) u_rj + conj(sum_{r-j=-m} conj(phi_r) u_rj)
                double tre[D], tim[D];
#pragma unroll
                for (int m = 0; m < D; ++m) tre[m] = tim[m] = 0.0;
#pragma unroll
                for (int r = 0; r < D; ++r) {
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        if (r == j) continue;
                        const int m = r > j ? r - j : j - r;
                        tre[m] = fma(f[r].re, u[r][j].re, tre[m]);
                        tre[m] = fma(f[r].im, u[r][j].im, tre[m]);
                        if (r > j) {
                            tim[m] = fma(f[r].re, u[r][j].im, tim[m]);
                            tim[m] = fma(-f[r].im, u[r][j].re, tim[m]);
                        } else {
                            tim[m] = fma(-f[r].re, u[r][j].im, tim[m]);
                            tim[m] = fma(f[r].im, u[r][j].re, tim[m]);
                        }
                    }
                }
#pragma unroll
                for (int m = 1; m < D; ++m) {
                    c = fma(rh[m].re, tre[m], c);
                    c = fma(-rh[m].im, tim[m], c);
                }
            } else {  // sum_{r != j} Re(conj(phi_r) u_rj f_rj)
#pragma unroll
                for (int r = 0; r < D; ++r) {
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        if (r == j) continue;
                        const cd z = cmulf(cconj(f[r]), u[r][j]), g = gauge_fd_weight<D>(fw, r, j);
                        c = fma(z.re, g.re, c);
                        c = fma(-z.im, g.im, c);
                    }
                }
            }
            const double sv = c * inv_eps;
            tot += sv;
            one = sv;
#pragma unroll
            for (int r = 0; r < D; ++r) {  // psi <- E psi
                cd s = u[r][0];
#pragma unroll
                for (int j = 1; j < D; ++j) s = cadd(s, u[r][j]);
                psi[w][r] = s;
            }
        }
    }
    return NSEC > 1 ? tot : one;
}
// the rank-one walk's chunk start of one sector: psi = Carry e_c, phi = Carry conj(m), m = row c of the sector's M
// block (of the twins' summed block: Mw2).  c is launch-uniform and enters addresses only.
template <int D>
__device__ __forceinline__ void merged_r1_init(const cd *ca, size_t nbe, const cd *Mw, const cd *Mw2, int c,
                                               cd (&psi)[D], cd (&phi)[D]) {
    cd m[D];
#pragma unroll
    for (int e = 0; e < D; ++e) m[e] = cconj(Mw2 ? cadd(Mw[c * D + e], Mw2[c * D + e]) : Mw[c * D + e]);
#pragma unroll
    for (int j = 0; j < D; ++j) {
        cd s = czero();
#pragma unroll
        for (int e = 0; e < D; ++e) cmac(s, ca[(size_t)(j * D + e) * nbe], m[e]);
        phi[j] = s;
        psi[j] = ca[(size_t)(j * D + c) * nbe];
    }
}
// One time-reversed gradient step of the wide pass, NSEC sectors over NE propagators, general charges (ladder
// charges: wide_step_grad_frame below): from psi_k and phi_k
//   psi_{k-1} = E_k^dag psi_k;   v_rj = conj(phi_k,r) (E_k)_rj;   the step's term sum_{r != j} Re(v_rj psi_{k-1},j f_rj)
//   over 1 / eps, as merged_step_grad_r1;   phi_{k-1},j = conj(sum_r v_rj)
// (The diagonal v_jj enter only phi's column sum; as a complex MAC onto the off-diagonal terms they are 10 F64
// instructions fewer per step and lane, which bought 0.8 % of the gradient walk and nothing that the bench could
// tell from its run-to-run spread: DESIGN.md 9.)
// The difference weights come in formed (wide_fd_weights): fw[we] the pair weights of propagator we.
template <int D, int NE, int NSEC>
__device__ __forceinline__ double wide_step_grad(const cd *Et, const GaugeN<D> (&gn)[NE], cd p1,
                                                 const cd (&fw)[NE][kGaugePairs<D>], double inv_eps,
                                                 cd (&psi)[NSEC][D], cd (&phi)[NSEC][D]) {
    constexpr int NSH = NSEC / NE;
    MStore<D, false> E[NE];
#pragma unroll
    for (int w = 0; w < NE; ++w) {
        cd dph[kGaugePairs<D>];
        gauge_phases<D>(p1, gn[w], dph);
        gauge_prop_lds<D, true>(Et + w * D * D, dph, E[w]);
    }
    double tot = 0.0, one = 0.0;
#pragma unroll
    for (int we = 0; we < NE; ++we) {
#pragma unroll
        for (int t = 0; t < NSH; ++t) {
            const int w = we * NSH + t;
            cd pm[D], v[D][D];
#pragma unroll
            for (int j = 0; j < D; ++j) {  // psi_{k-1} = E^dag psi_k
                cd s = czero();
#pragma unroll
                for (int r = 0; r < D; ++r) cmac(s, cconj(E[we].at(r, j)), psi[w][r]);
                pm[j] = s;
            }
#pragma unroll
            for (int r = 0; r < D; ++r) {
#pragma unroll
                for (int j = 0; j < D; ++j) v[r][j] = cmulf(cconj(phi[w][r]), E[we].at(r, j));
            }
            double c = 0.0;
#pragma unroll
            for (int r = 0; r < D; ++r) {  // sum_{r != j} Re(v_rj psi_j f_rj)
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    if (r == j) continue;
                    const cd z = cmulf(v[r][j], pm[j]), g = gauge_fd_weight<D>(fw[we], r, j);
                    c = fma(z.re, g.re, c);
                    c = fma(-z.im, g.im, c);
                }
            }
            const double sv = c * inv_eps;
            tot += sv;
            one = sv;
#pragma unroll
            for (int j = 0; j < D; ++j) {  // phi_{k-1} = E^dag phi_k = conj of the column sums of v
                cd s = v[0][j];
#pragma unroll
                for (int r = 1; r < D; ++r) s = cadd(s, v[r][j]);
                phi[w][j] = cconj(s);
                psi[w][j] = pm[j];
            }
        }
    }
    return NSEC > 1 ? tot : one;
}
// The same step in the step frame (ladder charges).  With chi = D_k^dag psi_k and eta = D_k^dag phi_k,
//   chi' = D_k^dag psi_{k-1} = E~^dag chi,   eta' = D_k^dag phi_{k-1} = E~^dag eta,
//   conj(phi_k,r) (E_k)_rj psi_{k-1},j = conj(eta_r) E~_rj chi'_j   entry by entry (the phases p_k^r p_k^-j cancel),
// so the step is wide_step_grad's with E~ for E_k and (eta, chi') for (phi, psi): E_k is never formed (36 VALU
// instructions and 52 registers for one 3-level and one 2-level propagator), and E~'s entries are the scalar
// operands of the products themselves (per-step scalar loads, as wide_step_frame).  The caller re-frames chi and
// eta from step k + 1's frame before the step (wide_reframe by dl = e^{i a (x_{k+1} - x_k)}).  The same quantity as
// wide_step_grad, other roundings.
template <int D, int NE, int NSEC, int DR>
__device__ __forceinline__ double wide_step_grad_frame(const cd *Et, const cd (&rh)[DR], double inv_eps,
                                                       cd (&chi)[NSEC][D], cd (&eta)[NSEC][D]) {
    static_assert(D <= DR, "weights up to the sector's highest charge difference");
    constexpr int NSH = NSEC / NE;
    double tot = 0.0, one = 0.0;
#pragma unroll
    for (int we = 0; we < NE; ++we) {
        cptr<cd> g = as_constant(Et + we * D * D);
        asm volatile("" : "+s"(g));
#pragma unroll
        for (int t = 0; t < NSH; ++t) {
            const int w = we * NSH + t;
            cd pm[D], v[D][D];
#pragma unroll
            for (int j = 0; j < D; ++j) {  // chi' = E~^dag chi
                cd s = czero();
#pragma unroll
                for (int r = 0; r < D; ++r) cmac(s, cconj(cload(g, r * D + j)), chi[w][r]);
                pm[j] = s;
            }
#pragma unroll
            for (int r = 0; r < D; ++r) {
#pragma unroll
                for (int j = 0; j < D; ++j) v[r][j] = cmulf(cconj(eta[w][r]), cload(g, r * D + j));
            }
            double tre[D], tim[D];  // T_m = sum_{r-j=m} v_rj chi'_j + conj(sum_{r-j=-m} v_rj chi'_j)
#pragma unroll
            for (int m = 0; m < D; ++m) tre[m] = tim[m] = 0.0;
#pragma unroll
            for (int r = 0; r < D; ++r) {
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    if (r == j) continue;
                    const int m = r > j ? r - j : j - r;
                    tre[m] = fma(v[r][j].re, pm[j].re, tre[m]);
                    tre[m] = fma(-v[r][j].im, pm[j].im, tre[m]);
                    if (r > j) {
                        tim[m] = fma(v[r][j].re, pm[j].im, tim[m]);
                        tim[m] = fma(v[r][j].im, pm[j].re, tim[m]);
                    } else {
                        tim[m] = fma(-v[r][j].re, pm[j].im, tim[m]);
                        tim[m] = fma(-v[r][j].im, pm[j].re, tim[m]);
                    }
                }
            }
            double c = 0.0;
#pragma unroll
            for (int m = 1; m < D; ++m) {
                c = fma(rh[m].re, tre[m], c);
                c = fma(-rh[m].im, tim[m], c);
            }
            const double sv = c * inv_eps;
            tot += sv;
            one = sv;
#pragma unroll
            for (int j = 0; j < D; ++j) {  // eta' = E~^dag eta = conj of the column sums of v
                cd s = v[0][j];
#pragma unroll
                for (int r = 1; r < D; ++r) s = cadd(s, v[r][j]);
                eta[w][j] = cconj(s);
                chi[w][j] = pm[j];
            }
        }
    }
    return NSEC > 1 ? tot : one;
}
// The wide gradient walk's difference weights (grape_fd_weight.hpp): the per-step phase a ((x_k + eps) - x_k) is
// a eps up to the rounding of x_k + eps, so the weights at phi0 = fl(a eps) are formed once per kernel -- by cis_m1
// and the recurrences the other walks run per step -- and a step adds the first-order term in dh = h - eps,
// h = (x_k + eps) - x_k: two FMAs per weight where cis_m1 and the recurrence take 28 VALU instructions.  h == eps
// gives dh = 0 and the per-step form's bits; a |dh| above the guard's bound (fd_threshold_h) takes the per-step form
// itself, in a divergent branch.  The base is the same in every lane: rho0 and the bound are wave-uniform scalars.
// An FMA reads one scalar operand, so the twin ladder form keeps its four derivative factors in vector registers (as
// scalars each is moved per use: 4 VALU instructions a step); the other forms hold them as scalars too and pay the
// moves (in vector registers they put the walk into scratch: 12 bytes a lane without twins, more with general
// charges' ten factors).
// Weights: ladder charges m = 1 .. DA - 1 (class B's one pair is m = 1); otherwise class A's pairs, then one pair per
// propagator of class B, each from its runtime charge difference.
__device__ __forceinline__ double wide_uniform(double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
template <int DA, int NEB, bool LAD>
struct WideFd {
    static constexpr int NW = LAD ? DA - 1 : kGaugePairs<DA> + NEB;
    double eps, thr;       // the guard: |h - eps| <= thr
    grape_fd::Base b[NW];  // rho0 and a g (fd_base_h)
};
template <int DA, int NEB, bool LAD>
__device__ __forceinline__ void wide_fd_base(double a, double eps, const GaugeN<DA> (&gA)[1], const GaugeN<2> (&gB)[NEB],
                                             WideFd<DA, NEB, LAD> &fd) {
    static_assert(DA >= 2, "class B's pair reads rho(1)");
    const cd q0 = cis_m1(a * eps);
    int mmax = 0;
    auto take = [&](int i, cd f, int dn) {
        const grape_fd::Base b = grape_fd::fd_base_h(grape_fd::fd_base_signed(grape_fd::Z{f.re, f.im}, dn), a);
        fd.b[i].rho0 = grape_fd::Z{wide_uniform(b.rho0.re), wide_uniform(b.rho0.im)};
        fd.b[i].g = (LAD && NEB == 1) ? b.g : grape_fd::Z{wide_uniform(b.g.re), wide_uniform(b.g.im)};
        mmax = max(mmax, dn < 0 ? -dn : dn);
    };
    if constexpr (LAD) {
        cd rh0[DA];
        ladder_rho<DA>(q0, rh0);
#pragma unroll
        for (int m = 1; m < DA; ++m) take(m - 1, rh0[m], m);
    } else {
        cd f0[kGaugePairs<DA>], f1[1];
        gauge_fd_weights_dn<DA>(q0, gA[0], f0);
#pragma unroll
        for (int r = 0; r < DA; ++r) {
#pragma unroll
            for (int j = r + 1; j < DA; ++j) take(gauge_pair(DA, r, j), f0[gauge_pair(DA, r, j)], gA[0].n[r] - gA[0].n[j]);
        }
#pragma unroll
        for (int w = 0; w < NEB; ++w) {
            gauge_fd_weights_dn<2>(q0, gB[w], f1);
            take(kGaugePairs<DA> + w, f1[0], gB[w].n[0] - gB[w].n[1]);
        }
    }
    fd.eps = eps;
    fd.thr = wide_uniform(grape_fd::fd_threshold_h(a, eps, mmax));
}
template <int DA, int NEB, bool LAD>
__device__ __forceinline__ void wide_fd_weights(const WideFd<DA, NEB, LAD> &fd, double a, double h, const GaugeN<DA> (&gA)[1],
                                                const GaugeN<2> (&gB)[NEB], cd (&rh)[DA], cd (&fwA)[1][kGaugePairs<DA>],
                                                cd (&fwB)[NEB][1]) {
    const double dh = h - fd.eps;
    auto at = [&](int i) {
        const grape_fd::Z z = grape_fd::fd_step(fd.b[i], dh);
        return cmake(z.re, z.im);
    };
    if (fabs(dh) <= fd.thr) {
        if constexpr (LAD) {
            rh[0] = czero();
#pragma unroll
            for (int m = 1; m < DA; ++m) rh[m] = at(m - 1);
        } else {
#pragma unroll
            for (int i = 0; i < kGaugePairs<DA>; ++i) fwA[0][i] = at(i);
#pragma unroll
            for (int w = 0; w < NEB; ++w) fwB[w][0] = at(kGaugePairs<DA> + w);
        }
    } else {  // the per-step form: x_k + eps rounded to x_k or to x_k + 2 eps, a NaN, or no bound for this a eps
        const cd q = cis_m1(a * h);
        if constexpr (LAD) {
            ladder_rho<DA>(q, rh);
        } else {
            gauge_fd_weights_dn<DA>(q, gA[0], fwA[0]);
#pragma unroll
            for (int w = 0; w < NEB; ++w) gauge_fd_weights_dn<2>(q, gB[w], fwB[w]);
        }
    }
}
// the wide gradient walk's start of one sector: psi_N as the forward walk left it (wide_store_psi),
// phi_N = conj(alpha) e_c (alpha: the head's factor of row c of M, grape_projector.hip k_wide_head; summed over a
// twin pair: a2)
template <int D>
__device__ __forceinline__ void wide_grad_init(const cd *u, size_t nbe, const cd *a, const cd *a2, int c, cd (&psi)[D],
                                               cd (&phi)[D]) {
    const cd al = cconj(a2 ? cadd(*a, *a2) : *a);
#pragma unroll
    for (int j = 0; j < D; ++j) {
        psi[j] = u[j * nbe];
        phi[j] = j == c ? al : czero();
    }
}
template <int DA, bool TWB, bool LAD>
__device__ __forceinline__ void wide_grad_body(const DevProblem &PA, const DevBatch &BA, const DevProblem &PB,
                                               const DevBatch &BB, double (*ftile)[kFdxTile + 1], int2 *frow,
                                               const grape_cis::CisTabEntry *ctab) {
    constexpr int NEB = TWB ? 1 : 2;
    constexpr int NXB = (TWB && GRAPE_WALK_TWIN_SUM) ? 1 : 2;
    const WideLane L = wide_lane(BA);
    frow[threadIdx.x] = make_int2(L.ok ? L.be : -1, 0);
    cd psiA[1][DA], phiA[1][DA], psiB[NXB][2], phiB[NXB][2];
    const size_t be = (size_t)L.be;
    const size_t nbe = (size_t)L.nbe;
    wide_grad_init<DA>(BA.Ub + be, nbe, BA.Msec + be, nullptr, PA.rank1_c[0], psiA[0], phiA[0]);
#pragma unroll
    for (int w = 0; w < NXB; ++w) {  // (twin sum: alpha_0 + alpha_1, both sectors' level at one index)
        const cd *ab = BB.Msec + be * 2 + w;
        wide_grad_init<2>(BB.Ub + (size_t)(TWB ? 0 : w) * 2 * nbe + be, nbe, ab, NXB == 1 ? ab + 1 : nullptr, PB.rank1_c[w],
                          psiB[w], phiB[w]);
    }
    GaugeN<DA> gA[1];
    GaugeN<2> gB[NEB];
    gA[0] = gauge_charges<DA>(PA, 0);
#pragma unroll
    for (int w = 0; w < NEB; ++w) gB[w] = gauge_charges<2>(PB, w);
    WideFd<DA, NEB, LAD> fd;
    wide_fd_base<DA, NEB, LAD>(PA.gauge_a, PA.eps, gA, gB, fd);
    // Ladder charges: the walk runs in the step frame (wide_step_grad_frame).  psi and phi hold chi = D^dag psi and
    // eta = D^dag phi in the frame of the step walked last -- the lab frame before the first one, as psi_N is stored
    // and phi_N is formed: x "of the step before" starts at 0 -- and a step re-frames both by
    // dl = e^{i a (xlast - x_k)} before its products.  xlast is the lane's own register: the tile slot it came from
    // holds the step's F_dx value by then, and the tile itself is replaced at a seam.
    double xlast = 0.0;
    auto step = [&](double xk) {  // one step of both classes: the F_dx value, in the plan's class order
        const double xe = xk + PA.eps;
        cd rh[DA], fwA[1][kGaugePairs<DA>], fwB[NEB][1];
        if constexpr (LAD) {
            cd pw[DA];
            ladder_powers<DA>(gauge_cis_tab(PA.gauge_a * (xlast - xk), ctab), pw);
            xlast = xk;
            wide_fd_weights<DA, NEB, LAD>(fd, PA.gauge_a, xe - xk, gA, gB, rh, fwA, fwB);  // (xe - xk: exact)
            wide_reframe<DA, 1>(pw, psiA);
            wide_reframe<DA, 1>(pw, phiA);
            wide_reframe<2, NXB>(pw, psiB);
            wide_reframe<2, NXB>(pw, phiB);
            const double sa = wide_step_grad_frame<DA, 1, 1>(PA.gauge_Et, rh, PA.inv_eps, psiA, phiA);
            const double sb = wide_step_grad_frame<2, NEB, NXB>(PB.gauge_Et, rh, PB.inv_eps, psiB, phiB);
            return sa + sb;
        } else {
            const cd p1 = gauge_cis_tab(PA.gauge_a * xk, ctab);
            wide_fd_weights<DA, NEB, LAD>(fd, PA.gauge_a, xe - xk, gA, gB, rh, fwA, fwB);  // (xe - xk: exact)
            const double sa = wide_step_grad<DA, 1, 1>(PA.gauge_Et, gA, p1, fwA, PA.inv_eps, psiA, phiA);
            const double sb = wide_step_grad<2, NEB, NXB>(PB.gauge_Et, gB, p1, fwB, PB.inv_eps, psiB, phiB);
            return sa + sb;  // (the classes' parts in either order: see k_walk_grad_m's step)
        }
    };
    // The tiles and the steps of a tile in descending order.  One workgroup tile serves both ways: it arrives
    // holding the tile's controls (wide_load_x), each lane replaces x_k in its row by the step's F_dx value, and the
    // flush writes the rows out as k_walk_grad_m's does (slot t of the tile is step j0 + t).
    const int jlast = (PA.Nt - 1) / kFdxTile * kFdxTile;
    const bool full = wide_group_full(L.nbe);
    const unsigned off = wide_tile_offset(PA.nx);
    const size_t row0 = (size_t)blockIdx.x * kWalkBlock * PA.nx;  // the workgroup's first row of x and of F_dx
    WideStamp stamp;  // (empty but in the diagnostic build)
    stamp.begin();
#pragma unroll 1
    for (int j0 = jlast; j0 >= 0; j0 -= kFdxTile) {
        const int nj = min(kFdxTile, PA.Nt - j0);
        const bool fast = full && j0 + kFdxTile <= PA.Nt;  // (workgroup-uniform)
        wide_set_prio((jlast - j0) / kFdxTile, jlast / kFdxTile + 1);
        if (fast) wide_load_x_full(ftile, BA.x + row0 + j0, PA.nx, off);
        else wide_load_x(ftile, BA.x, PA.nx, L.nbe, j0, PA.Nt);
        __syncthreads();
        stamp.seam_out();
#pragma unroll 1
        for (int t = nj - 1; t >= 0; --t) ftile[threadIdx.x][t] = step(ftile[threadIdx.x][t]);
        stamp.seam_in();
        __syncthreads();
        if (fast) {
            wide_flush_full(ftile, BA.Fdx + row0 + j0, PA.nx, off);
        } else {
            const int j = threadIdx.x % kFdxTile;
#pragma unroll 1
            for (int row = threadIdx.x / kFdxTile; row < kWalkBlock; row += kWalkBlock / kFdxTile) {
                const int br = frow[row].x;  // (br < 0: past the last lane)
                if (j < nj && br >= 0) BA.Fdx[(size_t)br * PA.nx + j0 + j] = ftile[row][j];
            }
        }
        __syncthreads();
    }
    wide_reset_prio();
    stamp.end(1);
}
template <int DA, bool TWB, bool LAD, bool R1, bool WIDE = false>
__global__ __launch_bounds__(kWalkBlock, (WIDE ? GRAPE_WALK_WIDE_GRAD_WAVES : R1 ? GRAPE_WALK_R1_WAVES : GRAPE_WALK_MERGED_WAVES)) void k_walk_grad_m(DevProblem PA, DevBatch BA,
                                                                                   DevProblem PB, DevBatch BB) {
    constexpr int NEB = TWB ? 1 : 2;
    __shared__ double ftile[kWalkBlock][kFdxTile + 1];  // (the F_dx tile; +1: conflict-free rows)
    __shared__ int2 frow[kWalkBlock];                   // each row's evaluation and first step
    __shared__ grape_cis::CisTabEntry ctab[grape_cis::kCisTabN];
    gauge_cis_stage(ctab);
    if constexpr (WIDE) {
        wide_grad_body<DA, TWB, LAD>(PA, BA, PB, BB, ftile, frow, ctab);
        return;
    }
    const VBlock vb = hw_block();
    const WalkLane L = walk_lane<1>(PA, BA, vb);
    const double *xt = BA.x + (size_t)L.be * PA.nx;  // this evaluation's row of x
    frow[threadIdx.x] = make_int2(L.ok ? L.be : -1, L.c * PA.L);
    // Twin class B (one propagator for both sectors): X_w <- E X_w E^dag is linear and the lane sums
    // the sectors' terms, so ONE state X = Carry (M_00 + M_11) Carry^dag carries both (GRAPE_WALK_TWIN_SUM:
    // half of class B's products; the sectors' sum formed once instead of per step -- rounding only)
    constexpr int NXB = (TWB && GRAPE_WALK_TWIN_SUM) ? 1 : 2;
    cd XA[1][DA][DA], XB[NXB][2][2];                          // the matrix walk's states
    cd psiA[1][DA], phiA[1][DA], psiB[NXB][2], phiB[NXB][2];  // the rank-one walk's (R1: X = psi phi^dag)
    if constexpr (R1) {
        const size_t nbe = (size_t)L.nbe, be = (size_t)L.be;
        merged_r1_init<DA>(BA.Carry + (size_t)L.c * DA * DA * nbe + be, nbe, BA.Msec + be * DA * DA, nullptr, PA.rank1_c[0],
                           psiA[0], phiA[0]);
#pragma unroll
        for (int w = 0; w < NXB; ++w) {  // (twin sum: m = m_0 + m_1, both sectors' level at one index)
            const cd *mb = BB.Msec + (be * 2 + w) * 4;
            merged_r1_init<2>(BB.Carry + ((size_t)(TWB ? 0 : w) * PB.nchunks + L.c) * 4 * nbe + be, nbe, mb,
                              NXB == 1 ? mb + 4 : nullptr, PB.rank1_c[w], psiB[w], phiB[w]);
        }
    } else {  // carries lane-minor (k_scan_seq), the head's M blocks row-major per sub-evaluation
        const size_t nbe = (size_t)L.nbe, be = (size_t)L.be;
        cd Cr[DA * DA];
        const cd *ca = BA.Carry + (size_t)L.c * DA * DA * nbe + be;
#pragma unroll
        for (int e = 0; e < DA * DA; ++e) Cr[e] = ca[(size_t)e * nbe];
        merged_xinit<DA>(Cr, BA.Msec + be * DA * DA, XA[0]);
#pragma unroll
        for (int w = 0; w < NXB; ++w) {
            cd Cb[4], Mb[4];
            const cd *cb = BB.Carry + ((size_t)(TWB ? 0 : w) * PB.nchunks + L.c) * 4 * nbe + be;
            const cd *mb = BB.Msec + (be * 2 + w) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                Cb[e] = cb[(size_t)e * nbe];
                Mb[e] = NXB == 1 ? cadd(mb[e], mb[4 + e]) : mb[e];
            }
            merged_xinit<2>(Cb, Mb, XB[w]);
        }
    }
    // E~: the rank-one walk's through scalar loads, the matrix walk's from LDS (gauge_prop_lds)
    const cd *EtA = R1 ? PA.gauge_Et
                       : gauge_base_lds<DA, 1>(PA, as_constant(PA.ops), BA.wscr + (size_t)L.slot * 2 * DA * DA);
    const cd *EtB = R1 ? PB.gauge_Et
                       : gauge_base_lds<2, NEB>(PB, as_constant(PB.ops), BB.wscr + (size_t)L.slot * 2 * 2 * 4);
    GaugeN<DA> gA[1];
    GaugeN<2> gB[NEB];
    gA[0] = gauge_charges<DA>(PA, 0);
#pragma unroll
    for (int w = 0; w < NEB; ++w) gB[w] = gauge_charges<2>(PB, w);
    const int k0 = L.c * PA.L;
    X2 xn = walk_load_x(1, xt + (size_t)min(k0, PA.Nt - 1));
    auto step = [&](int jj) {  // one step of both classes: the F_dx value, in the plan's class order
        const int k = min(k0 + jj, PA.Nt - 1);
        const double xk = xn.v0, xe = xk + PA.eps;  // the reference's perturbed control
        xn = walk_load_x(1, xt + (size_t)min(k + 1, PA.Nt - 1));  // next step's control
        const cd p1 = gauge_cis_tab(PA.gauge_a * xk, ctab), q = cis_m1(PA.gauge_a * (xe - xk));  // (xe - xk: exact)
        double sa, sb;
        if constexpr (R1) {
            sa = merged_step_grad_r1<DA, 1, 1, LAD>(EtA, gA, p1, q, PA.inv_eps, psiA, phiA);
            sb = merged_step_grad_r1<2, NEB, NXB, LAD>(EtB, gB, p1, q, PB.inv_eps, psiB, phiB);
        } else {
            sa = merged_step_grad<DA, 1, 1, LAD>(EtA, gA, p1, q, PA.inv_eps, XA);
            sb = merged_step_grad<2, NEB, NXB, LAD>(EtB, gB, p1, q, PB.inv_eps, XB);
        }
        // k_sec_reduce's sum of the classes' parts, (0 + part_0) + part_1 in the plan's class order: whichever class
        // is the plan's first, that is sa + sb -- 0 + a is a, addition commutes in IEEE arithmetic, and the one
        // exception (0 + -0 = +0) only turns a -0 sum of two -0 parts into +0, the same value -- so the lane adds
        // once instead of selecting the order (4 v_cndmask and an add per step)
        return sa + sb;
    };
    // F_dx straight to its [evaluation][n_x] row through a workgroup tile of kFdxTile steps: the
    // lanes of a workgroup hold consecutive evaluations, so a flush writes 16 lanes' kFdxTile-long
    // row pieces per instruction (no part array, no k_sec_reduce).  Uniform trip counts: every
    // lane reaches the barriers; steps past N_t are walked and not stored.
#pragma unroll 1
    for (int j0 = 0; j0 < PA.L; j0 += kFdxTile) {
        const int nj = min(kFdxTile, PA.L - j0);
#pragma unroll 1  // (unrolled by 2: the same instructions per step)
        for (int t = 0; t < nj; ++t) ftile[threadIdx.x][t] = step(j0 + t);
        __syncthreads();
        const int j = threadIdx.x % kFdxTile;
#pragma unroll 1
        for (int row = threadIdx.x / kFdxTile; row < kWalkBlock; row += kWalkBlock / kFdxTile) {
            const int br = frow[row].x, kk = frow[row].y + j0 + j;  // (br < 0: past the last lane)
            if (j < nj && br >= 0 && kk < PA.Nt) BA.Fdx[(size_t)br * PA.nx + kk] = ftile[row][j];
        }
        __syncthreads();
    }
}

}  // namespace grape
