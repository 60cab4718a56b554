// grape_walk_gauge.hpp -- helpers of the phase-covariant classes (a piece of grape_walk.hpp): the charges
// (GaugeN), the per-step phase base (gauge_cis, gauge_cis_tab, cis_m1), the pair phases and difference weights (gauge_phases,
// gauge_fd_weights_dn and their ladder forms), E~ of a workgroup's sectors (gauge_base, gauge_base_lds) and
// E_k = D_k E~ D_k^dag (gauge_sandwich, gauge_prop).  No kernel lives here; the chunk, merged, image and
// lab-frame walks and grape_eval1.hip all take their phases and products from this file, so kernels that share
// a phase base agree bit for bit (the merged family has its own, gauge_cis_tab).  The products of the phases with
// each other and with E~ are fused (cmulf): the reference never forms D_k E~ D_k^dag, so there is no product of
// its own to mirror, and the fused form has one rounding fewer per component.
#pragma once
#include "grape_cis.hpp"
#include "grape_fd_weight.hpp"
#include "grape_walk_core.hpp"

namespace grape {

// ---------------------------------------------------------------------------
// Phase-covariant classes (P.gauge, round 5): E_k = D_k E~ D_k^dag
// ---------------------------------------------------------------------------
// A control that enters H only as a phase -- the laser phase phi of the Rydberg models
// (RydbergTools.jl:31-130: e^{-i phi} Omega / 2 on every |1> -> |r> coupling) -- obeys
// H(x) = D(a x) H(0) D(a x)^dag, D(t) = diag(e^{i t N_j}) with integer charges N_j (the Rydberg
// excitation number).  The engine checks this per sector at plan creation (find_gauge: every entry
// of every sector block is e^{i a x (N_j - N_k)} times its value at x = 0).  Then
//   E_k = exp(-i dt H(x_k)) = D_k E~ D_k^dag,   E~ = exp(-i dt H(0))    (exactly, for any x_k)
// and the eps-variant of the step is E'_k = D'_k E~ D'_k^dag with D'_k = D_k diag(e^{i phi N_j}),
// phi = a ((x_k + eps) - x_k).  So a lane computes ONE exponential (E~, at its start) instead of
// one per step and variant; per step it forms E_k from E~ and the D phases of its levels, and
//   (E'_k - E_k)_rj = E_rj (rho_r + conj(rho_j) + rho_r conj(rho_j)),   1 + rho_j = e^{i phi N_j},
// with f_rj computed without cancellation (gauge_fd_weights_dn), so the reference's forward difference
// (UnitaryCalculations.jl:48-56) is formed from the exact perturbed propagator: same quantity, less
// rounding noise than two separate exponentials.  The charges are wave-uniform (one sector per
// workgroup row: scalar loads), so the per-level powers below are scalar-uniform loops.
template <int D>
struct GaugeN {
    int n[D];
};
template <int D>
constexpr int kGaugePairs = D > 1 ? D * (D - 1) / 2 : 1;  // level pairs j < k of a sector
__host__ __device__ constexpr int gauge_pair(int D, int j, int k) {  // j < k, row-major pair order
    return j * D - j * (j + 1) / 2 + (k - j - 1);
}
template <int D>
__device__ __forceinline__ GaugeN<D> gauge_charges(const DevProblem &P, int w) {
    const cptr<int> g = as_constant(P.gauge_n) + (size_t)w * D;
    GaugeN<D> r;
#pragma unroll
    for (int j = 0; j < D; ++j) r.n[j] = g[j];
    return r;
}
// z^n for a small wave-uniform n >= 0 (n - 1 complex products; exact 1 for n = 0)
__device__ __forceinline__ cd gauge_pow(cd z, int n) {
    cd r = cmake(1.0, 0.0);
    if (n > 0) r = z;
#pragma unroll 1
    for (int m = 1; m < n; ++m) r = cmulf(r, z);
    return r;
}
// p = e^{i t}: the per-step phase base of the phase-covariant walks (grape_cis.hpp: Cody-Waite reduction
// and fdlibm kernels, at most 1 unit of 2^-52 (tests/test_cis_cpu.py); the library sincos above |t| = 1e5).  Every
// gauge kernel outside the merged family (forward, gradient, image walk, eval1) takes its phases here, so the walks
// of one evaluation agree bit for bit.
// the constants of grape_cis::cis_fast as opaque SGPR pairs: an empty asm hides the literal from the
// instruction selector, so each Horner step is one v_fma_f64 with a scalar operand (not a v_fmac_f64 on
// a VGPR copy of the literal, two v_mov_b32 per constant and step: the walks are built without
// MachineLICM, so nothing is hoisted).  Not volatile: the asm stays free to move and to merge.
struct CisConst {
    __device__ __forceinline__ double operator()(int i) const {
        double v = grape_cis::kCisCoef[i];
        asm("" : "+s"(v));
        return v;
    }
};
__device__ __forceinline__ cd gauge_cis(double t) {
    double s, c;
    if (fabs(t) <= grape_cis::kCisFast) grape_cis::cis_fast(t, s, c, CisConst());
    else sincos(t, &s, &c);
    return cmake(c, s);
}
// The merged walks' p = e^{i t} (grape_cis::cis_tab: reduction by pi / 64, a 128-entry table, two short
// polynomials; the library sincos above |t| = 5e4): 28 VALU instructions where gauge_cis takes 46, a fifth of a wide
// step's.  Every form of k_walk_fwd_m / k_walk_grad_m takes its phase here and no other kernel does, so the merged
// family agrees with itself bit for bit and with the other families to rounding.  gauge_cis_stage copies the table
// (2 KB) from global memory to the workgroup's LDS before the first step; every lane of the workgroup must call it.
static __device__ const grape_cis::CisTabEntry kCisTableDev[grape_cis::kCisTabN] = {GRAPE_CIS_TABLE_ENTRIES};
__device__ __forceinline__ void gauge_cis_stage(grape_cis::CisTabEntry *tab) {
    for (int i = threadIdx.x; i < grape_cis::kCisTabN; i += blockDim.x) tab[i] = kCisTableDev[i];
    __syncthreads();
}
__device__ __forceinline__ cd gauge_cis_tab(double t, const grape_cis::CisTabEntry *tab) {
    double s, c;
    if (fabs(t) <= grape_cis::kCisTabFast) grape_cis::cis_tab(t, tab, s, c, CisConst());
    else sincos(t, &s, &c);
    return cmake(c, s);
}
// e^{i phi} - 1 without cancellation (grape_fd_weight.hpp, which a host compiler builds too: Taylor for the
// FD-sized phases, the library otherwise)
// (round 5: Horner in t^2 with the reciprocal factorials as constants -- the quotient form spent
// 8 double divisions per step, ~7 % of the merged gradient walk's VALU instructions)
__device__ __forceinline__ cd cis_m1(double phi) {
    const grape_fd::Z q = grape_fd::cis_m1(phi);
    return cmake(q.re, q.im);
}
// the difference weights of (E' - E)_rj = E_rj f_rj, formed once per pair r < j (f_jr = conj(f_rj) bit for bit),
// straight from the charge differences: f_rj = e^{i phi (N_r - N_j)} - 1 = rho(N_r - N_j) with
// rho(m) = (1 + q)^m - 1 by rho <- rho + q + q rho (no cancellation; rho(1) = q exactly), conjugated for N_r < N_j
template <int D>
__device__ __forceinline__ void gauge_fd_weights_dn(cd q, const GaugeN<D> &g, cd (&f)[kGaugePairs<D>]) {
#pragma unroll
    for (int r = 0; r < D; ++r) {
#pragma unroll
        for (int j = r + 1; j < D; ++j) {
            const int dn = g.n[r] - g.n[j], m = dn < 0 ? -dn : dn;
            cd z = q;
#pragma unroll 1
            for (int i = 1; i < m; ++i) z = cadd(cadd(z, q), cmulf(q, z));
            f[gauge_pair(D, r, j)] = m == 0 ? czero() : cmake(z.re, dn < 0 ? -z.im : z.im);
        }
    }
}
template <int D>
__device__ __forceinline__ cd gauge_fd_weight(const cd (&f)[kGaugePairs<D>], int r, int j) {
    return r < j ? f[gauge_pair(D, r, j)] : cconj(f[gauge_pair(D, j, r)]);
}
// E~ = exp(-i dt H_w(0)) of the workgroup's NE sectors (the nominal build at x = 0; no diagonal shift,
// so E~ carries its own phase), into every lane's Et.  Every lane of a workgroup walks the same
// sectors (walk_lane: w0 = NS * blockIdx.y), so lane w < NE computes sector w's exponential into LDS
// once for the whole workgroup -- the same code, hence the same bits, in the forward and the
// gradient walk.  (Every lane of the workgroup reaches the barrier: the pair kernels give each
// workgroup to one class.)
template <int D, int NE>
__device__ __forceinline__ void gauge_base(const DevProblem &P, cptr<cd> ops, cd *scr, cd (&Et)[NE][D][D]) {
    __shared__ cd gE[NE * D * D];
    if ((int)threadIdx.x < NE) {
        const int w = threadIdx.x;
        WalkX X0;
        X0.k0 = X0.k1 = X0.a0 = X0.a1 = 0.0;
        Pert none;
        none.var = -1;
        none.index = 0;
        none.delta = 0.0;
        SM<D> A[1];
        walk_build<D, 1>(P, ops + (size_t)w * P.sec_ops, X0, 1, none, A);
        double mu0 = 0.0;
        walk_expm<D, false, false>(A[0], scr, mu0, true, [&](int i, const cd (&x)[D]) {
#pragma unroll
            for (int j = 0; j < D; ++j) gE[(w * D + j) * D + i] = x[j];
        });
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NE; ++w) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
#pragma unroll
            for (int i = 0; i < D; ++i) Et[w][j][i] = gE[(w * D + j) * D + i];
        }
    }
}
// gauge_base without the register copy: E~ of the workgroup's NE sectors stays in LDS, row-major
// [w][D][D] (the merged walks read it at every step: 52 VGPRs fewer at DA = 3)
template <int D, int NE>
__device__ __forceinline__ const cd *gauge_base_lds(const DevProblem &P, cptr<cd> ops, cd *scr) {
    __shared__ cd gE[NE * D * D];
    if ((int)threadIdx.x < NE) {
        const int w = threadIdx.x;
        WalkX X0;
        X0.k0 = X0.k1 = X0.a0 = X0.a1 = 0.0;
        Pert none;
        none.var = -1;
        none.index = 0;
        none.delta = 0.0;
        SM<D> A[1];
        walk_build<D, 1>(P, ops + (size_t)w * P.sec_ops, X0, 1, none, A);
        double mu0 = 0.0;
        walk_expm<D, false, false>(A[0], scr, mu0, true, [&](int i, const cd (&x)[D]) {
#pragma unroll
            for (int j = 0; j < D; ++j) gE[(w * D + j) * D + i] = x[j];
        });
    }
    __syncthreads();
    return gE;
}
// The pair phases e_jk = e^{i theta (N_j - N_k)}, j < k (gauge_pair order), of one
// sector from p = e^{i theta}: p^|N_j - N_k| (|N_j - N_k| - 1 products, exactly 1 for equal charges),
// conjugated when N_j < N_k.  Round 5: E_jk = E~_jk e_jk and e_kj = conj(e_jk) take one complex
// product per off-diagonal element where d_j E~_jk conj(d_k) from the level phases took two.
template <int D>
__device__ __forceinline__ void gauge_phases(cd p, const GaugeN<D> &g, cd (&e)[kGaugePairs<D>]) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
#pragma unroll
        for (int k = j + 1; k < D; ++k) {
            const int dn = g.n[j] - g.n[k];
            const cd z = gauge_pow(p, dn < 0 ? -dn : dn);
            e[gauge_pair(D, j, k)] = cmake(z.re, dn < 0 ? -z.im : z.im);
        }
    }
}
// d_j M_jk conj(d_k) = M_jk e_jk (e_jj = 1: the diagonal unchanged)
template <int D>
__device__ __forceinline__ cd gauge_sandwich(const cd (&e)[kGaugePairs<D>], int j, int k, cd m) {
    return j == k ? m : j < k ? cmulf(m, e[gauge_pair(D, j, k)]) : cmulf(m, cconj(e[gauge_pair(D, k, j)]));
}
// E_k = D_k E~ D_k^dag; the diagonal is E~'s own
template <int D, class Store>
__device__ __forceinline__ void gauge_prop(const cd (&Et)[D][D], const cd (&e)[kGaugePairs<D>], Store &E) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
#pragma unroll
        for (int k = 0; k < D; ++k) E.set(j, k, gauge_sandwich<D>(e, j, k, Et[j][k]));
    }
}

// Ladder charges N_j = j (DevProblem::gauge_ladder, round 6): the pair phases e_jk = conj(p^{k-j}) and the
// difference weights f_rj = conj(rho(j - r)) (r < j) from compile-time charge differences -- the products
// of gauge_phases / gauge_fd_weights_dn in the same order (same bits), without their scalar loops over
// runtime charge differences
template <int D>
__device__ __forceinline__ void ladder_powers(cd z, cd (&pw)[D]) {  // pw[m] = z^m (gauge_pow's product order)
    pw[0] = cmake(1.0, 0.0);
#pragma unroll
    for (int m = 1; m < D; ++m) pw[m] = m == 1 ? z : cmulf(pw[m - 1], z);
}
template <int D>
__device__ __forceinline__ void ladder_rho(cd q, cd (&rh)[D]) {  // rho(m) = (1 + q)^m - 1 (gauge_fd_weights_dn)
    rh[0] = czero();
#pragma unroll
    for (int m = 1; m < D; ++m) rh[m] = m == 1 ? q : cadd(cadd(rh[m - 1], q), cmulf(q, rh[m - 1]));
}
template <int D>
__device__ __forceinline__ void gauge_phases_ladder(cd p, cd (&e)[kGaugePairs<D>]) {
    cd pw[D];
    ladder_powers<D>(p, pw);
#pragma unroll
    for (int j = 0; j < D; ++j) {
#pragma unroll
        for (int k = j + 1; k < D; ++k) e[gauge_pair(D, j, k)] = cconj(pw[k - j]);
    }
}

}  // namespace grape
