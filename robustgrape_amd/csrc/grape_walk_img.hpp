// grape_walk_img.hpp -- error sources through local-frame images (a piece of grape_walk.hpp): the image walk
// (k_walk_img; k_walk_img_gauge for a phase-covariant class) and its back end over the lane-minor images
// (k_walk_img_sum, k_walk_err_grad).  It serves classes whose error sources are not phase-covariant and plans
// with GRAPE_OPT_NO_GAUGE; covariant classes take the lab-frame walks (grape_walk_lab.hpp) by default.
#pragma once
#include "grape_walk_core.hpp"
#include "grape_walk_gauge.hpp"

namespace grape {

// ---------------------------------------------------------------------------
// Error sources: the image walk (k_walk_img, stage 0) and its F_dx traces (k_img_fdx, stage 1)
// ---------------------------------------------------------------------------
// With error sources the error kernels (grape_errpath.hpp: k_err_scan, k_err_grad) consume, per
// step, the local-frame images Y(dX) = Q_k^dag dX Q_{k-1} of every finite difference dX:
//   Z1_u = Y((E(x_u + eps) - E) / eps),  W_e = Y((E(err_e eps) - E) / eps),
//   Z2_{e,u} = Y((E(x_u + eps2, err_e eps2) + E - E(err_e eps2) - E(x_u + eps2)) / eps2^2)
// (UnitaryCalculations.jl:48-95).  Round 2 stored every variant propagator of the step (k_expm:
// 15 at C3) and Q_k (k_scan), and read them back (k_err_local): 2.95 MB of E per evaluation
// written and re-read.  The image walk forms the images in the lane that walks the chunk:
// per step the nominal E_k, then every variant's exponential column by column, its difference
// column dX e_i and at once column i of Z = E_k^dag dX, then
//   Y = Q_k^dag dX Q_{k-1} = Q_{k-1}^dag Z Q_{k-1}      (Q_k = E_k Q_{k-1}, unitary)
// column by column into its Zl slot, and finally Q <- E_k Q.  Only the images (9 tiles per step
// at C3) and the chunk totals T_c (k_scan's input, as k_walk_fwd) reach HBM.  The eps2
// propagators E(x_u + eps2) and E(err_e eps2) that the mixed stencil needs stay in registers:
// the walk serves any number nvg of gradient parameters per step (controls, and x_add when H0 or
// Herror read it); round 3 served nvg == 1 only.
struct VArg {
    Pert p;
    int err;
    double errval;
};
__device__ __forceinline__ VArg vload(cptr<VSpec> p, int i) {
    VArg a;
    a.p.var = p[i].pert.var;
    a.p.index = p[i].pert.index;
    a.p.delta = p[i].pert.delta;
    a.err = p[i].err;
    a.errval = p[i].errval;
    return a;
}

// The images of the walk path (B.Zl), lane-minor like the stored propagators (B.Ew): element el of
// image slot of sector w (of the lane's NS) at step jj of the lane's chunk, lanes = the image walk's
// launch width (gx * kWalkBlock lanes: one per (chunk, evaluation), evaluation fastest).  A wave's
// store or load of one element is 64 consecutive complex values (1 KB).
template <int D, int NS>
__device__ __forceinline__ size_t img_index(const DevProblem &P, int vy, int jj, int w, int slot, int el, size_t lanes,
                                            size_t lane) {
    return (((((size_t)vy * P.L + jj) * NS + w) * P.nz + slot) * (D * D) + el) * lanes + lane;
}
// the image walk's launch width for nbe evaluations (walk_lane: per = nbe * nchunks lanes, padded)
__device__ __forceinline__ size_t img_lanes(const DevProblem &P, int nbe) {
    return ((size_t)nbe * P.nchunks + kWalkBlock - 1) / kWalkBlock * kWalkBlock;
}

enum { IMG_DIFF = 0, IMG_MIX = 1, IMG_KEEP_D2 = 2, IMG_KEEP_E2 = 3 };
template <int K>
struct ImgKind {
    static constexpr int value = K;
};

template <int D, int NS>
__global__ __launch_bounds__(kWalkBlock, (WalkCfg<D, NS>::WAVES_IMG)) void k_walk_img(DevProblem P, DevBatch B) {
    using C = WalkCfg<D, NS>;
    constexpr int TS = D * D;
    const VBlock vb = hw_block();
    const WalkLane L = walk_lane<NS>(P, B, vb);
    const size_t lanes = (size_t)vb.gx * kWalkBlock, lane = (size_t)vb.x * kWalkBlock + threadIdx.x;
    const int ns = P.nsec > 1 ? P.nsec : 1;
    const double *xt = B.x + (size_t)L.be * P.nx;  // this evaluation's row of x
    const cptr<cd> ops = as_constant(P.ops) + (size_t)L.w0 * P.sec_ops;
    const cptr<VSpec> vs = as_constant(P.vs);
    cd *scr = B.wscr + (size_t)L.slot * NS * 2 * TS;
    Pert none;
    none.var = -1;
    none.index = 0;
    none.delta = 0.0;
    WalkX X;
    walk_set_xa(X, walk_load_x(P.na, xt + (size_t)P.np * P.Nt));  // x_add
    const int k0 = L.c * P.L;
    X2 xn = walk_load_x(P.np, xt + (size_t)min(k0, P.Nt - 1) * P.np);
    // Q_{k-1} (chunk-local), E_k, and the step's eps2 propagators E(x + eps2), E(err_e eps2) (the
    // latter two in the lane's LDS slots at D = 4, where the registers run out)
    cd Q[NS][D][D], E[NS][D][D];
    WalkPhase ph[NS];
    double mu[NS];  // this step's diagonal shifts (every variant takes the nominal's)
    constexpr bool EL = C::IMG_LDS;
    MStore<D, EL> Ed2[NS], Ee2[NS];
    if constexpr (EL) {
        static_assert(NS == 1, "one pair of LDS slots per lane");
        __shared__ cd lds_d2[kWalkBlock * MStore<D, true>::kStride], lds_e2[kWalkBlock * MStore<D, true>::kStride];
        Ed2[0].p = MStore<D, true>::slot(lds_d2);
        Ee2[0].p = MStore<D, true>::slot(lds_e2);
    }
#pragma unroll
    for (int w = 0; w < NS; ++w) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
#pragma unroll
            for (int i = 0; i < D; ++i) Q[w][j][i] = cmake(i == j ? 1.0 : 0.0, 0.0);
        }
    }
#pragma unroll 1
    for (int jj = 0; jj < P.L; ++jj) {  // uniform trip count; steps past N_t store into the sink
        const int k = min(k0 + jj, P.Nt - 1);
        const bool act = L.ok && k0 + jj < P.Nt;
        walk_set_xk(X, xn);
        xn = walk_load_x(P.np, xt + (size_t)min(k + 1, P.Nt - 1) * P.np);  // next step's controls
        {
            SM<D> A[NS];
            walk_build<D, NS>(P, ops, X, k + 1, none, A);
#pragma unroll
            for (int w = 0; w < NS; ++w) {
                walk_expm<D, C::FENCE, C::SHIFT>(A[w], scr + (size_t)w * 2 * TS, mu[w], true, [&](int i, const cd (&x)[D]) {
#pragma unroll
                    for (int j = 0; j < D; ++j) E[w][j][i] = x[j];
                });
                if constexpr (C::SHIFT) ph[w].add(act ? mu[w] : 0.0);
            }
        }
        // one variant: its exponential, and (IMG_DIFF / IMG_MIX) the image of its difference to slot
        auto variant = [&](auto kind, int v, int slot) {
            constexpr int KIND = decltype(kind)::value;
            const VArg va = vload(vs, v);
            SM<D> A[NS];
            walk_build<D, NS>(P, ops, X, k + 1, va.p, A, va.err, va.errval);
#pragma unroll
            for (int w = 0; w < NS; ++w) {
                if constexpr (KIND == IMG_KEEP_D2 || KIND == IMG_KEEP_E2) {
                    walk_expm<D, C::FENCE, C::SHIFT>(A[w], scr + (size_t)w * 2 * TS, mu[w], false, [&](int i, const cd (&x)[D]) {
#pragma unroll
                        for (int j = 0; j < D; ++j) {
                            if constexpr (KIND == IMG_KEEP_D2) Ed2[w].set(j, i, x[j]);
                            else Ee2[w].set(j, i, x[j]);
                        }
                    });
                } else {
                    cd Z[D][D];  // E_k^dag dX, column by column as the variant's columns come out
                    walk_expm<D, C::FENCE, C::SHIFT>(A[w], scr + (size_t)w * 2 * TS, mu[w], false, [&](int i, const cd (&x)[D]) {
                        cd dx[D];
                        const auto &e2 = Ee2[w].opaque();  // (LDS reads issued here, not hoisted)
                        const auto &d2 = Ed2[w].opaque();
#pragma unroll
                        for (int r = 0; r < D; ++r) {
                            if constexpr (KIND == IMG_DIFF) dx[r] = cscale(P.inv_eps, csub(x[r], E[w][r][i]));  // (E' - E) / eps
                            else  // (E(u + eps2, err eps2) + E - E(err eps2) - E(u + eps2)) / eps2^2, left to right
                                dx[r] = cscale(P.inv_eps2sq, csub(csub(cadd(x[r], E[w][r][i]), e2.at(r, i)), d2.at(r, i)));
                        }
#pragma unroll
                        for (int j = 0; j < D; ++j) {
                            cd c = czero();
#pragma unroll
                            for (int r = 0; r < D; ++r) cmac(c, cconj(E[w][r][j]), dx[r]);
                            Z[j][i] = c;
                        }
                    });
                    // Y = Q^dag Z Q column by column: t = Z q_c, y = Q^dag t, lane-minor (img_index): each
                    // store one coalesced 1-KB row per wave (steps past N_t fill the padding rows)
                    cd *dst = B.Zl + img_index<D, NS>(P, vb.y, jj, w, slot, 0, lanes, lane);
#pragma unroll
                    for (int cc = 0; cc < D; ++cc) {
                        cd t[D];
#pragma unroll
                        for (int m = 0; m < D; ++m) {
                            cd c = czero();
#pragma unroll
                            for (int n = 0; n < D; ++n) cmac(c, Z[m][n], Q[w][n][cc]);
                            t[m] = c;
                        }
#pragma unroll
                        for (int r = 0; r < D; ++r) {
                            cd c = czero();
#pragma unroll
                            for (int m = 0; m < D; ++m) cmac(c, cconj(Q[w][m][r]), t[m]);
                            dst[(size_t)(r * D + cc) * lanes] = c;
                        }
                    }
                }
            }
        };
        // the variant table of grape_plan_create, for nvg gradient parameters u (controls, then x_add
        // when H0 / Herror read it).  The mixed stencil of (u, e) needs E(x_u + eps2) and E(err_e eps2)
        // at once: one of each is kept, so E(err_e eps2) is recomputed for every u > 0 (nvg = 1, C3:
        // exactly round 3's sequence, each exponential once)
#pragma unroll 1
        for (int u = 0; u < P.nvg; ++u) variant(ImgKind<IMG_DIFF>{}, P.off_dx + u, u);  // Z1_u
#pragma unroll 1
        for (int u = 0; u < P.nvg; ++u) {
            variant(ImgKind<IMG_KEEP_D2>{}, P.off_dx2 + u, 0);  // E(x_u + eps2)
#pragma unroll 1
            for (int e = 0; e < P.ne; ++e) {
                const int ve = P.off_err + e * P.err_stride;
                if (u == 0) variant(ImgKind<IMG_DIFF>{}, ve, P.nvg + e);                 // W_e
                variant(ImgKind<IMG_KEEP_E2>{}, ve + 1, 0);                              // E(err_e eps2)
                variant(ImgKind<IMG_MIX>{}, ve + 2 + u, P.nvg + P.ne + e * P.nvg + u);  // Z2_{e,u}
            }
        }
#pragma unroll
        for (int w = 0; w < NS; ++w) {
#pragma unroll
            for (int i = 0; i < D; ++i) {  // column i of E_k Q (in place: it reads only column i)
                cd q[D], t[D];
#pragma unroll
                for (int m = 0; m < D; ++m) q[m] = Q[w][m][i];
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    cd c = czero();
#pragma unroll
                    for (int m = 0; m < D; ++m) cmac(c, q[m], E[w][j][m]);
                    t[j] = c;
                }
#pragma unroll
                for (int j = 0; j < D; ++j)
                    Q[w][j][i] = cmake(act ? t[j].re : Q[w][j][i].re, act ? t[j].im : Q[w][j][i].im);
            }
        }
    }
    if (L.ok) {
#pragma unroll
        for (int w = 0; w < NS; ++w) {
            if constexpr (C::SHIFT) walk_phase<D>(ph[w], Q[w]);
            cd *dst = B.Tc + (((size_t)L.be * ns + L.w0 + w) * P.nchunks + L.c) * TS;  // row-major chunk total
#pragma unroll
            for (int j = 0; j < D; ++j) {
#pragma unroll
                for (int i = 0; i < D; ++i) dst[j * D + i] = Q[w][j][i];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// The image walk of a phase-covariant class (P.gauge with error sources, nvg = 1; round 5)
// ---------------------------------------------------------------------------
// With H0 and every Herror_e covariant under the same D(a x) (find_gauge: the C3 Rabi and detuning
// errors of the Rydberg models are), every variant propagator of a step is a phase sandwich of an
// x-independent matrix: E_k = D E0 D^dag, E(err_e eps) = D E_e1 D^dag, E(x + eps2, err_e eps2) =
// D'' E_e2 D''^dag ... with E0 = exp(A0), E_e1 = exp(A0 + eps A_e0), E_e2 = exp(A0 + eps2 A_e0) (A at
// x = 0).  So the images' kernels Z = E_k^dag dX (UnitaryCalculations.jl:48-95) are
//   Z1   = D (E0^dag (E0 o f1)) D^dag / eps                           f1 from (x + eps) - x
//   W_e  = D (E0^dag (E_e1 - E0) / eps) D^dag = D K_e D^dag           x-independent K_e
//   Z2_e = D (E0^dag ((E_e2 - E0) o f2)) D^dag / eps2^2                f2 from (x + eps2) - x
// with (M o f)_rj = M_rj (rho_r + conj(rho_j) + rho_r conj(rho_j)) as in the gradient walk: the
// mixed stencil's four-term difference becomes one product without cancellation.  The workgroup
// (all lanes one sector group: blockIdx.y) computes E0, K_e and E_e2 - E0 once into LDS (1 + 2 ne
// exponentials per sector, the first lanes in parallel); per step a lane forms D from its control's
// phase, Z1 and Z2_e with one product each, and every image Y = Q^dag Z Q with two, instead of
// 3 + 3 ne exponentials per step.  Images, chunk totals and their layouts are k_walk_img's.

template <int D, int NS>
__device__ __forceinline__ cd *img_gauge_base(cd *g, int w, int b) {  // matrix b of sector w, row-major
    return g + ((size_t)w * (1 + 2 * kGaugeMaxE) + b) * D * D;
}
template <int D, int NS>
constexpr int img_gauge_waves() { return D >= 4 ? 1 : D == 3 ? 2 : NS == 1 ? 3 : 2; }
template <int D, int NS>
__global__ __launch_bounds__(kWalkBlock, (img_gauge_waves<D, NS>())) void k_walk_img_gauge(DevProblem P, DevBatch B) {
    constexpr int TS = D * D;
    constexpr int NBM = 1 + 2 * kGaugeMaxE;
    const VBlock vb = hw_block();
    const WalkLane L = walk_lane<NS>(P, B, vb);
    const size_t lanes = (size_t)vb.gx * kWalkBlock, lane = (size_t)vb.x * kWalkBlock + threadIdx.x;
    const int ns = P.nsec > 1 ? P.nsec : 1, NE = P.ne;
    const double *xt = B.x + (size_t)L.be * P.nx;  // this evaluation's row of x
    __shared__ cd gbase[NS * NBM * TS];
    // --- the workgroup's x-independent bases: lane t < NS (1 + 2 NE) computes matrix (w, b) ---
    {
        const int t = threadIdx.x, nb = 1 + 2 * NE;
        if (t < NS * nb) {
            const int w = t / nb, b = t % nb;
            const int e = b == 0 ? -1 : b <= NE ? b - 1 : b - 1 - NE;
            const double ev = b == 0 ? 0.0 : b <= NE ? P.eps : P.eps2;
            WalkX X0;
            X0.k0 = X0.k1 = X0.a0 = X0.a1 = 0.0;
            Pert none;
            none.var = -1;
            none.index = 0;
            none.delta = 0.0;
            SM<D> A[1];
            walk_build<D, 1>(P, as_constant(P.ops) + (size_t)(L.w0 + w) * P.sec_ops, X0, 1, none, A, e, ev);
            double mu0 = 0.0;
            cd *dst = img_gauge_base<D, NS>(gbase, w, b);
            walk_expm<D, false, false>(A[0], B.wscr + (size_t)L.slot * NS * 2 * TS, mu0, true,
                                             [&](int i, const cd (&x)[D]) {
#pragma unroll
                                                 for (int j = 0; j < D; ++j) dst[j * D + i] = x[j];
                                             });
        }
        __syncthreads();
        // K_e = E0^dag (E_e1 - E0) / eps and M_e = E_e2 - E0, in place (lane (w, e) owns both)
        cd K[TS], Mm[TS];
        const bool own = t < NS * NE;
        const int w = own ? t / NE : 0, e = own ? t % NE : 0;
        if (own) {
            const cd *E0 = img_gauge_base<D, NS>(gbase, w, 0), *E1 = img_gauge_base<D, NS>(gbase, w, 1 + e),
                     *E2 = img_gauge_base<D, NS>(gbase, w, 1 + NE + e);
#pragma unroll
            for (int r = 0; r < D; ++r) {
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    cd acc = czero();
#pragma unroll
                    for (int m = 0; m < D; ++m) cmac(acc, cconj(E0[m * D + r]), csub(E1[m * D + c], E0[m * D + c]));
                    K[r * D + c] = cscale(P.inv_eps, acc);
                    Mm[r * D + c] = csub(E2[r * D + c], E0[r * D + c]);
                }
            }
        }
        __syncthreads();
        if (own) {
            cd *K1 = img_gauge_base<D, NS>(gbase, w, 1 + e), *M2 = img_gauge_base<D, NS>(gbase, w, 1 + NE + e);
#pragma unroll
            for (int q = 0; q < TS; ++q) {
                K1[q] = K[q];
                M2[q] = Mm[q];
            }
        }
        __syncthreads();
    }
    GaugeN<D> gn[NS];
#pragma unroll
    for (int w = 0; w < NS; ++w) gn[w] = gauge_charges<D>(P, L.w0 + w);
    const int k0 = L.c * P.L;
    X2 xn = walk_load_x(1, xt + (size_t)min(k0, P.Nt - 1));
    cd Q[NS][D][D];
#pragma unroll
    for (int w = 0; w < NS; ++w) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
#pragma unroll
            for (int i = 0; i < D; ++i) Q[w][j][i] = cmake(i == j ? 1.0 : 0.0, 0.0);
        }
    }
#pragma unroll 1
    for (int jj = 0; jj < P.L; ++jj) {  // uniform trip count; steps past N_t store into the padding rows
        const int k = min(k0 + jj, P.Nt - 1);
        const bool act = L.ok && k0 + jj < P.Nt;
        const double xk = xn.v0;
        xn = walk_load_x(1, xt + (size_t)min(k + 1, P.Nt - 1));  // next step's control
        const cd p1 = gauge_cis(P.gauge_a * xk);
        const cd q1 = cis_m1(P.gauge_a * ((xk + P.eps) - xk)), q2 = cis_m1(P.gauge_a * ((xk + P.eps2) - xk));
#pragma unroll
        for (int w = 0; w < NS; ++w) {
            cd d[kGaugePairs<D>], f1[kGaugePairs<D>], f2[kGaugePairs<D>];
            gauge_phases<D>(p1, gn[w], d);
            gauge_fd_weights_dn<D>(q1, gn[w], f1);
            gauge_fd_weights_dn<D>(q2, gn[w], f2);
            const cd *E0 = img_gauge_base<D, NS>(gbase, w, 0);
            // image of slot: Y = Q^dag (D Zt D^dag) Q, Zt given row-major (scaled by `sc`)
            auto emit = [&](const cd (&Zt)[D][D], int slot, double sc) {
                cd Z[D][D];
#pragma unroll
                for (int r = 0; r < D; ++r) {
#pragma unroll
                    for (int c = 0; c < D; ++c)
                        Z[r][c] = cscale(sc, gauge_sandwich<D>(d, r, c, Zt[r][c]));
                }
                cd *dst = B.Zl + img_index<D, NS>(P, vb.y, jj, w, slot, 0, lanes, lane);
#pragma unroll
                for (int cc = 0; cc < D; ++cc) {
                    cd tt[D];
#pragma unroll
                    for (int m = 0; m < D; ++m) {
                        cd c = czero();
#pragma unroll
                        for (int n = 0; n < D; ++n) cmac(c, Z[m][n], Q[w][n][cc]);
                        tt[m] = c;
                    }
#pragma unroll
                    for (int r = 0; r < D; ++r) {
                        cd c = czero();
#pragma unroll
                        for (int m = 0; m < D; ++m) cmac(c, cconj(Q[w][m][r]), tt[m]);
                        dst[(size_t)(r * D + cc) * lanes] = c;
                    }
                }
            };
            // E0^dag (M o f) for M = E0 (Z1) or E_e2 - E0 (Z2_e)
            auto kernel_f = [&](const cd *M, const cd (&fw)[kGaugePairs<D>], cd (&Zt)[D][D]) {
                cd Mf[D][D];
#pragma unroll
                for (int r = 0; r < D; ++r) {
#pragma unroll
                    for (int c = 0; c < D; ++c) Mf[r][c] = r == c ? czero() : cmul(M[r * D + c], gauge_fd_weight<D>(fw, r, c));
                }
#pragma unroll
                for (int r = 0; r < D; ++r) {
#pragma unroll
                    for (int c = 0; c < D; ++c) {
                        cd acc = czero();
#pragma unroll
                        for (int m = 0; m < D; ++m) cmac(acc, cconj(E0[m * D + r]), Mf[m][c]);
                        Zt[r][c] = acc;
                    }
                }
            };
            {  // Z1 (slot 0)
                cd Zt[D][D];
                kernel_f(E0, f1, Zt);
                emit(Zt, 0, P.inv_eps);
            }
#pragma unroll 1
            for (int e = 0; e < NE; ++e) {  // W_e (slot 1 + e) and Z2_e (slot 1 + NE + e)
                cd Zt[D][D];
                const cd *Ke = img_gauge_base<D, NS>(gbase, w, 1 + e);
#pragma unroll
                for (int r = 0; r < D; ++r) {
#pragma unroll
                    for (int c = 0; c < D; ++c) Zt[r][c] = Ke[r * D + c];
                }
                emit(Zt, 1 + e, 1.0);
                kernel_f(img_gauge_base<D, NS>(gbase, w, 1 + NE + e), f2, Zt);
                emit(Zt, 1 + NE + e, P.inv_eps2sq);
            }
            // Q <- E_k Q with E_k = D E0 D^dag (column by column, in place)
            cd E[D][D];
#pragma unroll
            for (int j = 0; j < D; ++j) {
#pragma unroll
                for (int m = 0; m < D; ++m) E[j][m] = gauge_sandwich<D>(d, j, m, E0[j * D + m]);
            }
#pragma unroll
            for (int i = 0; i < D; ++i) {
                cd qq[D], t[D];
#pragma unroll
                for (int m = 0; m < D; ++m) qq[m] = Q[w][m][i];
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    cd c = czero();
#pragma unroll
                    for (int m = 0; m < D; ++m) cmac(c, qq[m], E[j][m]);
                    t[j] = c;
                }
#pragma unroll
                for (int j = 0; j < D; ++j)
                    Q[w][j][i] = cmake(act ? t[j].re : Q[w][j][i].re, act ? t[j].im : Q[w][j][i].im);
            }
        }
    }
    if (L.ok) {
#pragma unroll
        for (int w = 0; w < NS; ++w) {
            cd *dst = B.Tc + (((size_t)L.be * ns + L.w0 + w) * P.nchunks + L.c) * TS;
#pragma unroll
            for (int j = 0; j < D; ++j) {
#pragma unroll
                for (int i = 0; i < D; ++i) dst[j * D + i] = Q[w][j][i];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// The image walk's back end (error sources, walk path): walks over the lane-minor images
// ---------------------------------------------------------------------------
// Stage 1, k_walk_img_sum: one lane per (chunk c, evaluation) as the image walk, its NS sectors: the chunk
// sums of the error images sum_{k in c} W_{e,k} to B.Wc ([sub-evaluation][ne][nchunks][D][D], row-major tiles:
// Phase A of k_err_scan, UnitaryCalculations.jl:112).  It reads only the W images (C3: 4 of the 9 tiles per
// step): the F_dx traces Re tr(M'_c Z1_u) are taken by k_walk_err_grad's e = 0 lanes, which read Z1 anyway.
template <int D, int NS>
__global__ __launch_bounds__(kWalkBlock, 2) void k_walk_img_sum(DevProblem P, DevBatch B) {
    constexpr int TS = D * D;
    const VBlock vb = hw_block();
    const WalkLane L = walk_lane<NS>(P, B, vb);
    const int ns = P.nsec > 1 ? P.nsec : 1;
    const size_t lanes = (size_t)vb.gx * kWalkBlock, lane = (size_t)vb.x * kWalkBlock + threadIdx.x;
    const int k0 = L.c * P.L;
#pragma unroll
    for (int w = 0; w < NS; ++w) {
        const size_t sub = (size_t)L.be * ns + L.w0 + w;
#pragma unroll 1
        for (int e = 0; e < P.ne; ++e) {
            cd acc[TS];
#pragma unroll
            for (int t = 0; t < TS; ++t) acc[t] = czero();
#pragma unroll 1
            for (int jj = 0; jj < P.L; ++jj) {  // the sums in step order; steps past N_t add nothing
                cd v[TS];
                const cd *Wk = B.Zl + img_index<D, NS>(P, vb.y, jj, w, P.nvg + e, 0, lanes, lane);
#pragma unroll
                for (int t = 0; t < TS; ++t) v[t] = Wk[(size_t)t * lanes];
                const bool act = k0 + jj < P.Nt;  // (uniform within a chunk's lanes)
#pragma unroll
                for (int t = 0; t < TS; ++t) acc[t] = act ? cadd(acc[t], v[t]) : acc[t];
            }
            if (L.ok) {
                cd *dst = B.Wc + ((sub * P.ne + e) * P.nchunks + L.c) * TS;
#pragma unroll
                for (int t = 0; t < TS; ++t) dst[t] = acc[t];
            }
        }
    }
}

// Stage 2, k_walk_err_grad: one lane per (chunk c, evaluation, error e), e fastest (the ne lanes of
// an evaluation share one wave, so its Z1 rows are fetched once), its NS sectors.  The B_k
// recurrence of k_err_grad (grape_errpath.hpp) in the lane's registers:
//   B = T_c M' - M' T_c + M' Ttot at the chunk start, then per step
//   Lambda = B - M' W_k,  F_d2err_dx[u, k] (sector part) = Re tr(Lambda Z1_{k,u}) + Re tr(M' Z2_{k,e,u}),
//   B <- Lambda + W_k M'                                 (UnitaryCalculations.jl:112-139,
//                                                         FidelityCalculations.jl:85-113)
// with M' = M'_{c,e}, T_c, Ttot from k_err_scan / k_sec_mc_err (B.Me), the images lane-minor.  The
// terms go lane-major to B.sec_part_err ([nsec][ne][Nt][nvg][nbe]).
template <int D, int NS>
__global__ __launch_bounds__(kWalkBlock, (D >= 4 ? 1 : 2)) void k_walk_err_grad(DevProblem P, DevBatch B) {
    constexpr int TS = D * D;
    const int ns = P.nsec > 1 ? P.nsec : 1;
    const int nbe = B.nb / ns;
    const long per = (long)nbe * P.nchunks;
    const long gtot = (long)blockIdx.x * kWalkBlock + threadIdx.x;
    const int e = (int)(gtot % P.ne);
    const long g = gtot / P.ne;  // the image walk's lane
    const bool ok = g < per;
    const long gg = ok ? g : 0;
    const int c = (int)(gg / nbe), be = (int)(gg - (long)c * nbe);
    const size_t lanes = img_lanes(P, nbe), lane = (size_t)gg;
    const int vy = blockIdx.y, w0 = vy * NS;
    const int k0 = c * P.L;
#pragma unroll
    for (int w = 0; w < NS; ++w) {
        const size_t sub = (size_t)be * ns + w0 + w;
        const cd *Mo = B.Me + ((sub * P.ne + e) * P.nchunks + c) * 3 * TS;  // M', T_c, Ttot
        cd Mp[TS], Bk[TS], T1[TS], T2[TS];
#pragma unroll
        for (int t = 0; t < TS; ++t) {
            Mp[t] = Mo[t];
            T1[t] = Mo[TS + t];
        }
        walk_mm<D>(T1, Mp, Bk);  // T_c M'
        walk_mm<D>(Mp, T1, T2);  // M' T_c
#pragma unroll
        for (int t = 0; t < TS; ++t) {
            Bk[t] = csub(Bk[t], T2[t]);
            T1[t] = Mo[2 * TS + t];
        }
        walk_mm<D>(Mp, T1, T2);  // M' Ttot
#pragma unroll
        for (int t = 0; t < TS; ++t) Bk[t] = cadd(Bk[t], T2[t]);
        const int w_slot = P.nvg + e, z2_slot = P.nvg + P.ne + e * P.nvg;
        cd Mc[TS];  // M'_c (F_dx; every e-lane of an evaluation loads the same rows, the e = 0 lane stores)
        {
            const cd *Mcp = B.Mc + (sub * P.nchunks + c) * TS;
#pragma unroll
            for (int t = 0; t < TS; ++t) Mc[t] = Mcp[t];
        }
#pragma unroll 1
        for (int jj = 0; jj < P.L; ++jj) {
            const int k = k0 + jj;
            const bool act = ok && k < P.Nt;
            cd Wk[TS];
            const cd *Wp = B.Zl + img_index<D, NS>(P, vy, jj, w, w_slot, 0, lanes, lane);
#pragma unroll
            for (int t = 0; t < TS; ++t) Wk[t] = Wp[(size_t)t * lanes];
#pragma unroll
            for (int t = 0; t < TS; ++t) {  // Lambda_k = B - M' W, in place (no product temporary)
                cd c = czero();
#pragma unroll
                for (int m = 0; m < D; ++m) cmac(c, Mp[(t / D) * D + m], Wk[m * D + t % D]);
                Bk[t] = csub(Bk[t], c);
            }
#pragma unroll 1
            for (int u = 0; u < P.nvg; ++u) {
                const cd *z1 = B.Zl + img_index<D, NS>(P, vy, jj, w, u, 0, lanes, lane);
                const cd *z2 = B.Zl + img_index<D, NS>(P, vy, jj, w, z2_slot + u, 0, lanes, lane);
                double s = 0.0;  // sum_i sum_j Lambda[i][j] Z1[j][i] + M'[i][j] Z2[j][i]
                double sdx = 0.0;  // F_dx: sum_i sum_j M'_c[i][j] Z1[j][i] (from the same Z1 loads)
#pragma unroll
                for (int i = 0; i < D; ++i) {
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        const cd a = z1[(size_t)(j * D + i) * lanes], bz = z2[(size_t)(j * D + i) * lanes];
                        s += Bk[i * D + j].re * a.re - Bk[i * D + j].im * a.im;
                        s += Mp[i * D + j].re * bz.re - Mp[i * D + j].im * bz.im;
                        sdx += Mc[i * D + j].re * a.re - Mc[i * D + j].im * a.im;
                    }
                }
                if (e == 0) {  // F_dx[u, k] (sector part) = Re tr(M'_c Z1_u)
                    double *dx = act ? B.sec_part + ((((size_t)(w0 + w) * P.Nt) + k) * P.nvg + u) * nbe + be
                                     : reinterpret_cast<double *>(B.sink);
                    *dx = sdx;
                }
                double *dst = act ? B.sec_part_err +
                                        (((((size_t)(w0 + w) * P.ne + e) * P.Nt + k) * P.nvg + u) * nbe + be)
                                  : reinterpret_cast<double *>(B.sink);
                *dst = s;
            }
#pragma unroll
            for (int t = 0; t < TS; ++t) {  // B_{k+1} = Lambda_k + W_k M', in place
                cd c = czero();
#pragma unroll
                for (int m = 0; m < D; ++m) cmac(c, Wk[(t / D) * D + m], Mp[m * D + t % D]);
                Bk[t] = cadd(Bk[t], c);
            }
        }
    }
}

}  // namespace grape
