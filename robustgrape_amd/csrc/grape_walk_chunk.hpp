// grape_walk_chunk.hpp -- the per-class chunk walks (a piece of grape_walk.hpp, whose overview derives them):
// one lane owns one (evaluation, chunk) of a sector class and walks the chunk's steps twice,
//   k_walk_fwd   E_k = exp(A_k) and the chain Q <- E_k Q in registers; writes the chunk total T_c
//   k_walk_grad  X = M'_c, then per step Y_k = X E_k^dag, F_dx[u,k] = Re tr(Y_k (E'_k - E_k) / eps), X <- E_k Y_k
// with recomputed or stored (B.Ew) propagators, twin sectors, and the phase-covariant form (GAUGE), and the
// pair kernels that run two classes' walks in one launch for latency-bound calls.
#pragma once
#include "grape_walk_core.hpp"
#include "grape_walk_gauge.hpp"

namespace grape {

// STORE: also hand the propagators to the gradient walk (B.Ew; P.walk_store_e)
// TWIN (P.twin, NS = 2): the lane's two sectors have identical operator blocks (e.g. the Rydberg
// sectors {01, 0r} and {10, r0} at equal Rabi frequencies and detunings): their propagators, chains
// and chunk totals are identical, so one exponential and one chain per step serve both.
// GAUGE: a phase-covariant class (P.gauge): E_k = D_k E~ D_k^dag from the lane's one exponential E~
template <int D, int NS, bool STORE, bool TWIN = false, bool GAUGE = false>
__device__ __forceinline__ void walk_fwd_body(const DevProblem &P, const DevBatch &B, const VBlock vb) {
    using C = WalkCfg<D, NS>;
    static_assert(!TWIN || (NS == 2 && !STORE), "twin sectors: two per lane, recomputed propagators");
    static_assert(!(GAUGE && STORE), "gauge classes form E_k from E~: nothing to store");
    constexpr int NE = TWIN ? 1 : NS;  // distinct propagators / chains per lane
    constexpr int TS = D * D;
    const WalkLane L = walk_lane<NS>(P, B, vb);
    const int ns = P.nsec > 1 ? P.nsec : 1;
    const double *xt = B.x + (size_t)L.be * P.nx;  // this evaluation's row of x
    const cptr<cd> ops = as_constant(P.ops) + (size_t)L.w0 * P.sec_ops;
    cd *scr = B.wscr + (size_t)L.slot * NS * 2 * TS;
    Pert none;
    none.var = -1;
    none.index = 0;
    none.delta = 0.0;
    const size_t lanes = (size_t)vb.gx * kWalkBlock, lane = (size_t)vb.x * kWalkBlock + threadIdx.x;
    MStore<D, false> E;
    WalkX X;
    walk_set_xa(X, walk_load_x(P.na, xt + (size_t)P.np * P.Nt));  // x_add
    const int k0 = L.c * P.L;
    X2 xn = walk_load_x(P.np, xt + (size_t)min(k0, P.Nt - 1) * P.np);
    cd Q[NE][D][D];
    WalkPhase ph[NE];
#pragma unroll
    for (int w = 0; w < NE; ++w) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
#pragma unroll
            for (int i = 0; i < D; ++i) Q[w][j][i] = cmake(i == j ? 1.0 : 0.0, 0.0);
        }
    }
    cd Et[GAUGE ? NE : 1][D][D];  // GAUGE: E~ of the lane's sectors
    GaugeN<D> gn[GAUGE ? NE : 1];
    if constexpr (GAUGE) {
        gauge_base<D, NE>(P, ops, scr, Et);
#pragma unroll
        for (int w = 0; w < NE; ++w) gn[w] = gauge_charges<D>(P, L.w0 + w);
    }
    constexpr bool SHIFT = C::SHIFT && !GAUGE;
#pragma unroll 1
    for (int jj = 0; jj < P.L; ++jj) {  // uniform trip count; steps past N_t leave Q alone
        const int k = min(k0 + jj, P.Nt - 1);
        const bool act = k0 + jj < P.Nt;
        walk_set_xk(X, xn);
        xn = walk_load_x(P.np, xt + (size_t)min(k + 1, P.Nt - 1) * P.np);  // next step's controls
        SM<D> A[GAUGE ? 1 : NE];
        cd p1 = czero();
        if constexpr (GAUGE) {
            p1 = gauge_cis(P.gauge_a * X.k0);  // e^{i a x_k}
        } else {
            walk_build<D, NE>(P, ops, X, k + 1, none, A);
        }
#pragma unroll
        for (int w = 0; w < NE; ++w) {
            double mu = 0.0;
            if constexpr (GAUGE) {
                cd dph[kGaugePairs<D>];
                gauge_phases<D>(p1, gn[w], dph);
                gauge_prop<D>(Et[w], dph, E);
            } else {
                walk_expm<D, C::FENCE, C::SHIFT>(A[w], scr + (size_t)w * 2 * TS, mu, true, [&](int i, const cd (&x)[D]) {
#pragma unroll
                    for (int j = 0; j < D; ++j) E.set(j, i, x[j]);
                });
            }
            if constexpr (SHIFT) ph[w].add(act ? mu : 0.0);
            if constexpr (STORE) {  // the gradient walk's copy: lane-minor, one coalesced 1-KB store per element
                cd *ew = B.Ew + ((((size_t)vb.y * P.L + jj) * NS + w) * kEwStride<D>) * lanes + lane;
#pragma unroll
                for (int j = 0; j < D; ++j) {
#pragma unroll
                    for (int i = 0; i < D; ++i) ew[(size_t)(j * D + i) * lanes] = E.at(j, i);
                }
                ew[(size_t)TS * lanes] = cmake(mu, 0.0);
            }
#pragma unroll
            for (int i = 0; i < D; ++i) {  // column i of E_k Q (in place: it reads only column i)
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
                for (int j = 0; j < D; ++j)
                    Q[w][j][i] = cmake(act ? t[j].re : Q[w][j][i].re, act ? t[j].im : Q[w][j][i].im);
            }
        }
    }
    if (L.ok) {
        if constexpr (SHIFT) {
#pragma unroll
            for (int w = 0; w < NE; ++w) walk_phase<D>(ph[w], Q[w]);
        }
#pragma unroll
        for (int w = 0; w < NS; ++w) {
            const int we = TWIN ? 0 : w;
            cd *dst = B.Tc + (((size_t)L.be * ns + L.w0 + w) * P.nchunks + L.c) * TS;  // row-major chunk total
#pragma unroll
            for (int j = 0; j < D; ++j) {
#pragma unroll
                for (int i = 0; i < D; ++i) dst[j * D + i] = Q[we][j][i];
            }
        }
    }
}

template <int D, int NS, bool STORE, bool TWIN = false, bool GAUGE = false>
__global__ __launch_bounds__(kWalkBlock, (GAUGE ? WalkCfg<D, NS>::WAVES_GAUGE : WalkCfg<D, NS>::WAVES_FWD))
void k_walk_fwd(DevProblem P, DevBatch B) {
    walk_fwd_body<D, NS, STORE, TWIN, GAUGE>(P, B, hw_block());
}

// STORED: the nominal propagators come from the forward walk's copy (B.Ew, prefetched one step
// ahead) instead of being recomputed -- one exponential of the three per step saved for 512 B of
// HBM traffic per step and sector.
// NVG: the number of gradient parameters when known at compile time (1: C1 / C2 / C4), else 0
// (a runtime loop) -- a static count of the F_dx stores per step keeps the prefetch waits exact.
// TWIN: one nominal and one eps-variant exponential per step serve both sectors of the lane (their
// X, Y and contractions stay per sector: M differs between them in general)
// GAUGE: a phase-covariant class (P.gauge; NVG == 1): E_k from E~ and the level phases, and the
// eps-variant's difference E' - E = E o f with f_rj = rho_r + conj(rho_j) + rho_r conj(rho_j)
// Several sectors per lane (NS > 1: the 2-level classes without error sources) write ONE F_dx part per lane
// row -- the sectors' terms summed in sector order -- so k_sec_reduce reads nsec / NS parts for that class
// (grape_walk_api.hpp grad_parts)
template <int D, int NS, bool STORED, int NVG, bool TWIN = false, bool GAUGE = false>
__device__ __forceinline__ void walk_grad_body(const DevProblem &P, const DevBatch &B, const VBlock vb) {
    using C = WalkCfg<D, NS>;
    static_assert(!TWIN || (NS == 2 && !STORED), "twin sectors: two per lane, recomputed propagators");
    static_assert(!GAUGE || (!STORED && NVG == 1), "gauge classes: recomputed propagators, one control");
    constexpr int NE = TWIN ? 1 : NS;     // distinct propagators per lane
    constexpr int NSH = TWIN ? NS : 1;    // sectors sharing each of them
    constexpr int TS = D * D;
    const WalkLane L = walk_lane<NS>(P, B, vb);
    const int ns = P.nsec > 1 ? P.nsec : 1;
    const double *xt = B.x + (size_t)L.be * P.nx;  // this evaluation's row of x
    const cptr<cd> ops = as_constant(P.ops) + (size_t)L.w0 * P.sec_ops;
    cd *scr = B.wscr + (size_t)L.slot * NS * 2 * TS;
    Pert none;
    none.var = -1;
    none.index = 0;
    none.delta = 0.0;
    // X_{k-1} = C_{k-1} M C_{k-1}^dag of every sector (M'_c at the chunk start); Y_k in place
    constexpr bool XL = C::X_LDS && !STORED;
    MStore<D, XL> X[NS];
    MStore<D, false> E[NE];
    if constexpr (XL) {
        static_assert(NS == 1, "one LDS slot per lane");
        __shared__ cd lds[kWalkBlock * MStore<D, true>::kStride];
        X[0].p = MStore<D, true>::slot(lds);
    }
    const size_t lanes = (size_t)vb.gx * kWalkBlock, lane = (size_t)vb.x * kWalkBlock + threadIdx.x;
    auto ew = [&](int jj, int w) { return B.Ew + ((((size_t)vb.y * P.L + jj) * NS + w) * kEwStride<D>) * lanes + lane; };
    cd En[STORED ? NS : 1][D][D];  // the next step's stored propagators (STORED)
    double mun[NS], mu[NE];        // ... and their shifts; this step's shifts
    if constexpr (STORED) {
#pragma unroll
        for (int w = 0; w < NS; ++w) {
            const cd *src = ew(0, w);
#pragma unroll
            for (int j = 0; j < D; ++j) {
#pragma unroll
                for (int i = 0; i < D; ++i) En[w][j][i] = src[(size_t)(j * D + i) * lanes];
            }
            mun[w] = src[(size_t)TS * lanes].re;
        }
    }
    // X = M'_c = Carry_c M_ww Carry_c^dagger from the carry and the head's sector block (k_sec_mc's
    // arithmetic, element by element: the same values, and one launch less per sector class)
#pragma unroll
    for (int w = 0; w < NS; ++w) {
        const size_t bw = (size_t)L.be * ns + L.w0 + w;
        const cd *Cr = B.Carry + (bw * P.nchunks + L.c) * TS, *Mw = B.Msec + bw * TS;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            cd r[D];  // column j of M_ww Carry^dagger
#pragma unroll
            for (int a = 0; a < D; ++a) {
                cd v = czero();
#pragma unroll
                for (int e = 0; e < D; ++e) v = cadd(v, cmul(Mw[a * D + e], cconj(Cr[j * D + e])));
                r[a] = v;
            }
#pragma unroll
            for (int i = 0; i < D; ++i) {
                cd acc = czero();
#pragma unroll
                for (int a = 0; a < D; ++a) acc = cadd(acc, cmul(Cr[i * D + a], r[a]));
                X[w].set(i, j, acc);
            }
        }
    }
    WalkX XV;
    walk_set_xa(XV, walk_load_x(P.na, xt + (size_t)P.np * P.Nt));
    const int k0 = L.c * P.L;
    X2 xn = walk_load_x(P.np, xt + (size_t)min(k0, P.Nt - 1) * P.np);
    const cptr<VSpec> vs = as_constant(P.vs);
    cd Et[GAUGE ? NE : 1][D][D];  // GAUGE: E~ of the lane's sectors (the forward walk's bits)
    GaugeN<D> gn[GAUGE ? NE : 1];
    cd fwp[GAUGE ? NE : 1][kGaugePairs<D>];  // GAUGE: this step's difference weights (gauge_fd_weights_dn)
    if constexpr (GAUGE) {
        gauge_base<D, NE>(P, ops, scr, Et);
#pragma unroll
        for (int w = 0; w < NE; ++w) gn[w] = gauge_charges<D>(P, L.w0 + w);
    }
#pragma unroll 1
    for (int jj = 0; jj < P.L; ++jj) {  // uniform trip count; steps past N_t store nothing
        const int k = min(k0 + jj, P.Nt - 1);
        const bool act = L.ok && k0 + jj < P.Nt;
        walk_set_xk(XV, xn);
        xn = walk_load_x(P.np, xt + (size_t)min(k + 1, P.Nt - 1) * P.np);  // next step's controls
        if constexpr (GAUGE) {
            const double xk = XV.k0, xe = xk + P.eps;  // the reference's perturbed control (Pert delta = eps)
            const cd p1 = gauge_cis(P.gauge_a * xk), q = cis_m1(P.gauge_a * (xe - xk));  // (xe - xk: exact)
#pragma unroll
            for (int w = 0; w < NE; ++w) {
                cd dph[kGaugePairs<D>];
                gauge_phases<D>(p1, gn[w], dph);
                gauge_prop<D>(Et[w], dph, E[w]);
                mu[w] = 0.0;
                gauge_fd_weights_dn<D>(q, gn[w], fwp[w]);
            }
        } else if constexpr (STORED) {  // this step's propagators; the next step's loads go out now
#pragma unroll
            for (int w = 0; w < NS; ++w) {
#pragma unroll
                for (int j = 0; j < D; ++j) {
#pragma unroll
                    for (int i = 0; i < D; ++i) E[w].set(j, i, En[w][j][i]);
                }
                mu[w] = mun[w];
            }
            const int jn = jj + 1 < P.L ? jj + 1 : jj;
#pragma unroll
            for (int w = 0; w < NS; ++w) {
                const cd *src = ew(jn, w);
#pragma unroll
                for (int j = 0; j < D; ++j) {
#pragma unroll
                    for (int i = 0; i < D; ++i) En[w][j][i] = src[(size_t)(j * D + i) * lanes];
                }
                mun[w] = src[(size_t)TS * lanes].re;
            }
        } else {
            SM<D> A[NE];
            walk_build<D, NE>(P, ops, XV, k + 1, none, A);
#pragma unroll
            for (int w = 0; w < NE; ++w)
                walk_expm<D, C::FENCE, C::SHIFT>(A[w], scr + (size_t)w * 2 * TS, mu[w], true, [&](int i, const cd (&x)[D]) {
#pragma unroll
                    for (int j = 0; j < D; ++j) E[w].set(j, i, x[j]);
                });
        }
        // Y = X E^dag, in place row by row (row r of Y reads row r of X only)
#pragma unroll
        for (int w = 0; w < NS; ++w) {
            const int we = TWIN ? 0 : w;
#pragma unroll
            for (int r = 0; r < D; ++r) {
                cd xr[D], y[D];
#pragma unroll
                for (int j = 0; j < D; ++j) xr[j] = X[w].at(r, j);
#pragma unroll
                for (int cc = 0; cc < D; ++cc) {
                    cd s = czero();
#pragma unroll
                    for (int j = 0; j < D; ++j) cmac(s, xr[j], cconj(E[we].at(cc, j)));
                    y[cc] = s;
                }
#pragma unroll
                for (int cc = 0; cc < D; ++cc) X[w].set(r, cc, y[cc]);
            }
        }
        if constexpr (GAUGE) {  // F_dx[k] = Re tr(Y (E' - E)) / eps with (E' - E)_rj = E_rj f_rj (f_jj = 0)
            double tot = 0.0;
#pragma unroll
            for (int we = 0; we < NE; ++we) {
                double s[NSH];
#pragma unroll
                for (int t = 0; t < NSH; ++t) s[t] = 0.0;
                const auto &Ej = E[we].opaque();
                const auto &fw = fwp[we];
#pragma unroll
                for (int r = 0; r < D; ++r) {
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        if (r == j) continue;
                        const cd de = cscale(P.inv_eps, cmul(Ej.at(r, j), gauge_fd_weight<D>(fw, r, j)));
#pragma unroll
                        for (int t = 0; t < NSH; ++t) {
                            const cd y = X[we * NSH + t].opaque().at(j, r);
                            s[t] = fma(y.re, de.re, s[t]);
                            s[t] = fma(-y.im, de.im, s[t]);
                        }
                    }
                }
#pragma unroll
                for (int t = 0; t < NSH; ++t) {
                    const int w = we * NSH + t;
                    if constexpr (NS > 1) {
                        tot += s[t];
                    } else {
                        double *dst = act ? B.sec_part + ((((size_t)(L.w0 + w) * P.Nt) + k) * P.nvg) * L.nbe + L.be
                                          : reinterpret_cast<double *>(B.sink);
                        *dst = s[t];
                    }
                }
            }
            if constexpr (NS > 1) {
                double *dst = act ? B.sec_part + ((((size_t)(L.w0 / NS) * P.Nt) + k) * P.nvg) * L.nbe + L.be
                                  : reinterpret_cast<double *>(B.sink);
                *dst = tot;
            }
        }
        // eps-variants: F_dx[u, k] = Re tr(Y (E' - E)) / eps, column j of E' against row j of Y
#pragma unroll 1
        for (int u = 0; u < (GAUGE ? 0 : NVG > 0 ? NVG : P.nvg); ++u) {
            SM<D> Ap[NE];
            walk_build<D, NE>(P, ops, XV, k + 1, pload(vs, P.off_dx + u), Ap);
            double tot = 0.0;  // (NS > 1: the lane's sectors summed, in sector order)
#pragma unroll
            for (int we = 0; we < NE; ++we) {
                double s[NSH];
#pragma unroll
                for (int t = 0; t < NSH; ++t) s[t] = 0.0;
                walk_expm<D, C::FENCE, C::SHIFT>(Ap[we], scr + (size_t)we * 2 * TS, mu[we], false, [&](int j, const cd (&x)[D]) {
                    if constexpr (NSH == 1) {
                        const auto &Yj = X[we].opaque();  // row j of Y and column j of E read here, after
                        const auto &Ej = E[we].opaque();  // column j of E'
#pragma unroll
                        for (int r = 0; r < D; ++r) {
                            const cd de = cscale(P.inv_eps, csub(x[r], Ej.at(r, j)));  // (1/eps) (E' - E)
                            const cd y = Yj.at(j, r);
                            s[0] = fma(y.re, de.re, s[0]);
                            s[0] = fma(-y.im, de.im, s[0]);
                        }
                    } else {  // twins: one difference column, contracted with each sector's row j of Y
                        const auto &Ej = E[we].opaque();
                        cd de[D];
#pragma unroll
                        for (int r = 0; r < D; ++r) de[r] = cscale(P.inv_eps, csub(x[r], Ej.at(r, j)));
#pragma unroll
                        for (int t = 0; t < NSH; ++t) {
                            const auto &Yj = X[we * NSH + t].opaque();
#pragma unroll
                            for (int r = 0; r < D; ++r) {
                                const cd y = Yj.at(j, r);
                                s[t] = fma(y.re, de[r].re, s[t]);
                                s[t] = fma(-y.im, de[r].im, s[t]);
                            }
                        }
                    }
                });
#pragma unroll
                for (int t = 0; t < NSH; ++t) {
                    const int w = we * NSH + t;
                    if constexpr (NS > 1) {
                        tot += s[t];
                    } else {
                        // unconditional store (inactive lanes write the sink): exact vmcnt accounting
                        double *dst = act ? B.sec_part + ((((size_t)(L.w0 + w) * P.Nt) + k) * P.nvg + u) * L.nbe + L.be
                                          : reinterpret_cast<double *>(B.sink);
                        *dst = s[t];
                    }
                }
            }
            if constexpr (NS > 1) {  // one part per lane row: index w0 / NS
                double *dst = act ? B.sec_part + ((((size_t)(L.w0 / NS) * P.Nt) + k) * P.nvg + u) * L.nbe + L.be
                                  : reinterpret_cast<double *>(B.sink);
                *dst = tot;
            }
        }
        // X <- E Y, in place column by column
#pragma unroll
        for (int w = 0; w < NS; ++w) {
            const int we = TWIN ? 0 : w;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                cd y[D], t[D];
#pragma unroll
                for (int m = 0; m < D; ++m) y[m] = X[w].at(m, i);
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    cd c = czero();
#pragma unroll
                    for (int m = 0; m < D; ++m) cmac(c, E[we].at(j, m), y[m]);
                    t[j] = c;
                }
#pragma unroll
                for (int j = 0; j < D; ++j) X[w].set(j, i, t[j]);
            }
        }
    }
}

template <int D, int NS, bool STORED, int NVG, bool TWIN = false, bool GAUGE = false>
__global__ __launch_bounds__(kWalkBlock, (GAUGE ? WalkCfg<D, NS>::WAVES_GAUGE
                                                : STORED ? WalkCfg<D, NS>::WAVES_GRAD_STORED : WalkCfg<D, NS>::WAVES_GRAD))
void k_walk_grad(DevProblem P, DevBatch B) {
    walk_grad_body<D, NS, STORED, NVG, TWIN, GAUGE>(P, B, hw_block());
}

// Pair kernels (latency-bound calls): two sector classes' walks in ONE launch -- the first
// n0 = gx0 * gy0 workgroups walk class 0 (D0, NS0; STORE0: its stored propagators), the rest class 1
// -- so a single evaluation's classes run side by side instead of one launch after the other
// (graph branches do not run concurrently on this runtime: scripts/probes/graph_branch_probe.hip).
// The registers are the larger class's; at these sizes the grid is a few workgroups.
// GA: both classes phase-covariant (P.gauge; then class 0 stores nothing)
template <int D0, int NS0, bool ST0, int D1, int NS1, bool TW1 = false, bool GA = false>
__global__ __launch_bounds__(kWalkBlock, 1) void k_walk_fwd_pair(DevProblem P0, DevBatch B0, DevProblem P1, DevBatch B1,
                                                                 int gx0, int gy0, int gx1) {
    const int id = blockIdx.x, n0 = gx0 * gy0;
    if (id < n0) walk_fwd_body<D0, NS0, ST0 && !GA, false, GA>(P0, B0, VBlock{id % gx0, id / gx0, gx0});
    else walk_fwd_body<D1, NS1, false, TW1, GA>(P1, B1, VBlock{(id - n0) % gx1, (id - n0) / gx1, gx1});
}
template <int D0, int NS0, bool ST0, int D1, int NS1, bool TW1 = false, bool GA = false>
__global__ __launch_bounds__(kWalkBlock, 1) void k_walk_grad_pair(DevProblem P0, DevBatch B0, DevProblem P1, DevBatch B1,
                                                                  int gx0, int gy0, int gx1) {
    const int id = blockIdx.x, n0 = gx0 * gy0;
    if (id < n0) walk_grad_body<D0, NS0, ST0 && !GA, 1, false, GA>(P0, B0, VBlock{id % gx0, id / gx0, gx0});
    else walk_grad_body<D1, NS1, false, 1, TW1, GA>(P1, B1, VBlock{(id - n0) % gx1, (id - n0) / gx1, gx1});
}

}  // namespace grape
