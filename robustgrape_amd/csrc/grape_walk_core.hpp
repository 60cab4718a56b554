// grape_walk_core.hpp -- what every walk family shares (a piece of grape_walk.hpp, which has the overview).
//
// The arithmetic of one step and the frame of one lane:
//   SM, sm_*, sm_regime, walk_expm    compressed (skew-)Hermitian matrices and the column-by-column exponential
//                                     (Taylor 6 / 9 / 12 by the shifted column bound; Taylor 30 and squaring above)
//   cptr, as_constant, cload, pload   launch-uniform problem data through the constant address space (scalar loads)
//   WalkX, walk_load_x, walk_build    the step's controls in registers and A_w = -i dt H_w(x_k) term by term
//   MStore                            a lane's D x D matrix in registers or in its private LDS slot
//   WalkLane, VBlock, walk_lane       launch geometry: one lane per (chunk, evaluation) and group of NS sectors
//   the knob block, WalkCfg           waves per SIMD of every walk kernel (the knobs stay together, here)
//   WalkPhase, walk_phase, kEwStride  the chunk's accumulated diagonal shift; the stored propagators' layout
//   walk_mm, merged_xinit             two D x D products that several families' chunk starts take
#pragma once
#include "grape_kernels.hpp"
#include "grape_walk_api.hpp"

namespace grape {

constexpr int kWalkBlock = kWalkBlockA;
// 1/k! as literals (the column kernels index them with compile-time constants)
__device__ __forceinline__ constexpr double inv_fact(int k) {
    return k == 0 ? 1.0 : k == 1 ? 1.0 : k == 2 ? 0.5 : k == 3 ? 1.0 / 6 : k == 4 ? 1.0 / 24 : k == 5 ? 1.0 / 120
         : k == 6 ? 1.0 / 720 : k == 7 ? 1.0 / 5040 : k == 8 ? 1.0 / 40320 : k == 9 ? 1.0 / 362880
         : k == 10 ? 1.0 / 3628800 : k == 11 ? 1.0 / 39916800 : 1.0 / 479001600;
}

// ---------------------------------------------------------------------------
// compressed (skew-)Hermitian matrices
// ---------------------------------------------------------------------------
template <int D>
struct SM {
    static constexpr int NU = D * (D - 1) / 2;
    double d[D];  // diagonal: imaginary parts (skew-Hermitian) or real parts (Hermitian)
    cd u[NU];     // strict upper triangle, row by row
};
__host__ __device__ constexpr int uix(int D, int j, int k) { return j * D - j * (j + 1) / 2 + (k - j - 1); }

// element (j, k) (compile-time indices after unrolling)
template <int D, bool HERM>
__device__ __forceinline__ cd sm_el(const SM<D> &M, int j, int k) {
    if (j == k) return HERM ? cmake(M.d[j], 0.0) : cmake(0.0, M.d[j]);
    if (j < k) return M.u[uix(D, j, k)];
    const cd t = M.u[uix(D, k, j)];
    return HERM ? cmake(t.re, -t.im) : cmake(-t.re, t.im);
}
// c += M[j][k] v: 2 FMAs for a diagonal entry, 4 otherwise
template <int D, bool HERM>
__device__ __forceinline__ void sm_mac(cd &c, const SM<D> &M, int j, int k, cd v) {
    if (j == k) {
        const double s = M.d[j];
        if (HERM) {
            c.re = fma(s, v.re, c.re);
            c.im = fma(s, v.im, c.im);
        } else {
            c.re = fma(-s, v.im, c.re);
            c.im = fma(s, v.re, c.im);
        }
    } else {
        cmac(c, sm_el<D, HERM>(M, j, k), v);
    }
}
template <int D, bool HERM>
__device__ __forceinline__ void sm_matvec(const SM<D> &M, const cd (&v)[D], cd (&out)[D]) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
        cd c = czero();
#pragma unroll
        for (int k = 0; k < D; ++k) sm_mac<D, HERM>(c, M, j, k, v[k]);
        out[j] = c;
    }
}

// A^2 (Hermitian) and A^3 = A A^2 (skew-Hermitian) of a skew-Hermitian A
template <int D>
__device__ __forceinline__ void sm_cube(const SM<D> &A, SM<D> &A2, SM<D> &A3) {
#pragma unroll
    for (int j = 0; j < D; ++j) {  // (A^2)_jj = -sum_m |A_jm|^2
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < D; ++m) {
            if (m == j) {
                s = fma(A.d[j], A.d[j], s);
            } else {
                const cd a = sm_el<D, false>(A, j, m);
                s = fma(a.re, a.re, s);
                s = fma(a.im, a.im, s);
            }
        }
        A2.d[j] = -s;
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
#pragma unroll
        for (int k = j + 1; k < D; ++k) {
            cd c = czero();
#pragma unroll
            for (int m = 0; m < D; ++m) sm_mac<D, false>(c, A, j, m, sm_el<D, false>(A, m, k));
            A2.u[uix(D, j, k)] = c;
        }
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {  // Im (A^3)_jj
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < D; ++m) {
            const cd b = sm_el<D, true>(A2, m, j);
            if (m == j) {
                s = fma(A.d[j], b.re, s);
            } else {
                const cd a = sm_el<D, false>(A, j, m);
                s = fma(a.re, b.im, s);
                s = fma(a.im, b.re, s);
            }
        }
        A3.d[j] = s;
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
#pragma unroll
        for (int k = j + 1; k < D; ++k) {
            cd c = czero();
#pragma unroll
            for (int m = 0; m < D; ++m) sm_mac<D, false>(c, A, j, m, sm_el<D, true>(A2, m, k));
            A3.u[uix(D, j, k)] = c;
        }
    }
}

// The high-norm regime (|A - i mu I|_1 > 0.25, where Julia's exp! takes Pade 7 / 9 / 13): Taylor 30
// (Paterson-Stockmeyer in A^3, kWalkNstHi = 9 Horner steps) of A / 2^s with s = max(0,
// ceil(log2(|A|_1 / kWalkThetaHi))) and s squarings.  The remainder at 3.2 is 3.2^31 / 31! = 6e-19;
// the measured errors of E, (E' - E) / eps and the eps2 mixed stencil against an extended-precision
// reference equal Julia's Pade 13 at every |A|_1 from 0.3 to 80 (scripts/probes/highnorm_study.py,
// DESIGN.md 4.2), where the round-3 Taylor 12 at 0.25 (s = ceil(log2 4|A|_1): 4 more squarings) was up
// to 10x worse.  Coefficients by index from constant memory (the Horner loop is not unrolled: a rare
// path, kept out of the common path's registers and code).
constexpr double kWalkThetaHi = 3.2;
constexpr int kWalkNstHi = 9;
__host__ __device__ constexpr double inv_fact_r(int k) { return k <= 1 ? 1.0 : inv_fact_r(k - 1) / k; }
static __constant__ double kWalkInvFact[3 * kWalkNstHi + 4] = {
    inv_fact_r(0),  inv_fact_r(1),  inv_fact_r(2),  inv_fact_r(3),  inv_fact_r(4),  inv_fact_r(5),  inv_fact_r(6),
    inv_fact_r(7),  inv_fact_r(8),  inv_fact_r(9),  inv_fact_r(10), inv_fact_r(11), inv_fact_r(12), inv_fact_r(13),
    inv_fact_r(14), inv_fact_r(15), inv_fact_r(16), inv_fact_r(17), inv_fact_r(18), inv_fact_r(19), inv_fact_r(20),
    inv_fact_r(21), inv_fact_r(22), inv_fact_r(23), inv_fact_r(24), inv_fact_r(25), inv_fact_r(26), inv_fact_r(27),
    inv_fact_r(28), inv_fact_r(29), inv_fact_r(30)};

// The top coefficients of a Paterson-Stockmeyer evaluation in A^3 with nst Horner steps
// (degree 3 nst + 3: nst = 1, 2, 3 -> Taylor 6, 9, 12)
__device__ __forceinline__ double ps_top(int nst, int m) {
    return nst == 1 ? inv_fact(3 + m) : nst == 2 ? inv_fact(6 + m) : inv_fact(9 + m);
}

// x = column i of the Taylor polynomial, Paterson-Stockmeyer in A^3 (grape_device.hpp
// expm_taylor): degree 3 nst + 3 (12, 9 or 6).  B_j = c_3j I + c_3j+1 A + c_3j+2 A^2.
template <int D>
__device__ __forceinline__ void sm_taylor_col(int nst, int i, const SM<D> &A, const SM<D> &A2, const SM<D> &A3,
                                              cd (&x)[D]) {
    {
        const double k0 = ps_top(nst, 0), k1 = ps_top(nst, 1), k2 = ps_top(nst, 2), k3 = ps_top(nst, 3);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            x[j] = caxpy(k1, sm_el<D, false>(A, j, i), caxpy(k2, sm_el<D, true>(A2, j, i), cscale(k3, sm_el<D, false>(A3, j, i))));
            if (j == i) x[j].re += k0;
        }
    }
#pragma unroll
    for (int st = 2; st >= 0; --st) {
        if (st == 0 || st < nst) {  // (the last step unconditionally: no branch around it)
            cd t[D];
            sm_matvec<D, false>(A3, x, t);
            const double k0 = inv_fact(3 * st), k1 = inv_fact(3 * st + 1), k2 = inv_fact(3 * st + 2);
#pragma unroll
            for (int j = 0; j < D; ++j) {
                x[j] = caxpy(k1, sm_el<D, false>(A, j, i), caxpy(k2, sm_el<D, true>(A2, j, i), t[j]));
                if (j == i) x[j].re += k0;
            }
        }
    }
    pin<D>(x);  // the column is final here: nothing of the next one is scheduled into it
}

// column i of the high-norm regime's Taylor 30 (a2: column i of A^2)
template <int D>
__device__ __forceinline__ void sm_taylor_col_hi(int i, const SM<D> &A, const SM<D> &A2, const SM<D> &A3, cd (&x)[D]) {
    cd a2[D];
#pragma unroll
    for (int j = 0; j < D; ++j) a2[j] = sm_el<D, true>(A2, j, i);
    constexpr int N = kWalkNstHi;
    {
        const double k0 = kWalkInvFact[3 * N], k1 = kWalkInvFact[3 * N + 1], k2 = kWalkInvFact[3 * N + 2],
                     k3 = kWalkInvFact[3 * N + 3];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            x[j] = caxpy(k1, sm_el<D, false>(A, j, i), caxpy(k2, a2[j], cscale(k3, sm_el<D, false>(A3, j, i))));
            if (j == i) x[j].re += k0;
        }
    }
#pragma unroll 1
    for (int st = N - 1; st >= 0; --st) {
        cd t[D];
        sm_matvec<D, false>(A3, x, t);
        const double k0 = kWalkInvFact[3 * st], k1 = kWalkInvFact[3 * st + 1], k2 = kWalkInvFact[3 * st + 2];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            x[j] = caxpy(k1, sm_el<D, false>(A, j, i), caxpy(k2, a2[j], t[j]));
            if (j == i) x[j].re += k0;
        }
    }
    pin<D>(x);
}

// Degree choice (grape_device.hpp expm_prologue_fast, per lane): 0 = diagonal (isdiag), 3 =
// Taylor 6, 4 = Taylor 9, 5 = Taylor 12, 13 = Taylor 30 of A / 2^s (A scaled here) and s squarings.
//
// Diagonal shift (SHIFT; WalkCfg::SHIFT): the walks exponentiate A - i mu I, i.e. they compute
// E~ = e^{-i mu} exp(A), with mu (`choose`) the midpoint of the diagonal's imaginary parts, which
// minimises the largest diagonal modulus -- the Rydberg 4-level sector (diagonal 0, 0, 0, B = 10)
// drops from |A|_1 ~ 0.17 to ~ 0.09 and takes Taylor 9 (two Horner steps per column instead of
// three).  The phase e^{i mu} is never multiplied in per step: every eps-variant of a step is
// shifted by the nominal propagator's mu (choose = false), so E' - E = e^{i mu} (E~' - E~) and the
// phase cancels in every sandwich the walks form (Y = X E^dag, X E^dag (E' - E), E X E^dag,
// E^dag dX); only the chunk totals take e^{i sum mu} (walk_phase).  The thresholds bound the
// Taylor remainder sum_{k > m} |A|^k / k! by ~3e-17 (0.015 at m = 6, 0.1 at m = 9; 2.4e-18 at
// 0.25, m = 12).  A diagonal A (kind 0) keeps mu = 0 when choosing, and so does an A whose shifted
// norm still exceeds 0.25 (the high-norm regime: no Horner step to save, more FD noise).
template <int D, bool SHIFT>
__device__ __forceinline__ int sm_regime(SM<D> &A, int &s, double &mu, bool choose) {
    s = 0;
    bool off = false;
#pragma unroll
    for (int t = 0; t < SM<D>::NU; ++t) off = off || A.u[t].re != 0.0 || A.u[t].im != 0.0;
    if (choose) {
        mu = 0.0;
        if (SHIFT && off) {
            double lo = A.d[0], hi = A.d[0];
#pragma unroll
            for (int j = 1; j < D; ++j) {
                lo = fmin(lo, A.d[j]);
                hi = fmax(hi, A.d[j]);
            }
            mu = 0.5 * (lo + hi);
            // Only where the shifted A stays in the Taylor 6 / 9 / 12 regime: above that the shift
            // saves no Horner step and its rounding raises the eps / eps2 stencils' noise (the
            // shifted Taylor 30 at |A|_1 = 2.6 ... 84 measured 3-10x Julia's error on F_dx and
            // F_d2err_dx against an extended-precision exponential, unshifted ~1x:
            // scripts/probes/shift_noise_study.py).
            double nsh = 0.0;
#pragma unroll
            for (int c = 0; c < D; ++c) {
                double ub = fabs(A.d[c] - mu);
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    if (j == c) continue;
                    const cd a = sm_el<D, false>(A, j, c);
                    ub += fabs(a.re) + fabs(a.im);
                }
                nsh = fmax(nsh, ub);
            }
            if (!(nsh <= 0.25)) mu = 0.0;
        }
    }
    if (!off) return 0;  // (walk_expm shifts the diagonal itself)
    if (SHIFT) {
#pragma unroll
        for (int j = 0; j < D; ++j) A.d[j] -= mu;  // exact for mu = 0
    }
    double nub = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        double ub = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const cd a = sm_el<D, false>(A, j, c);
            ub += fabs(a.re) + fabs(a.im);
        }
        nub = c == 0 ? ub : fmax(nub, ub);
    }
    if (nub <= 0.015) return 3;
    if (SHIFT && nub <= 0.1) return 4;
    if (nub <= 0.25) return 5;
    double nA = 0.0;  // Julia's opnorm(A, 1)
#pragma unroll
    for (int c = 0; c < D; ++c) {
        double cs = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const cd a = sm_el<D, false>(A, j, c);
            cs += sqrt(a.re * a.re + a.im * a.im);
        }
        nA = c == 0 ? cs : fmax(nA, cs);
    }
    if (nA <= 0.015) return 3;
    if (SHIFT && nA <= 0.1) return 4;
    if (nA <= 0.25) return 5;
    if (!(nA <= 1e300)) return 5;  // NaN / Inf: propagates through the polynomial
    s = nA <= kWalkThetaHi ? 0 : (int)ceil(log2(nA / kWalkThetaHi));  // |A / 2^s|_1 <= 3.2 (Taylor 30)
    const double f = ldexp(1.0, -s);  // exact
#pragma unroll
    for (int j = 0; j < D; ++j) A.d[j] *= f;
#pragma unroll
    for (int t = 0; t < SM<D>::NU; ++t) A.u[t] = cscale(f, A.u[t]);
    return 13;
}

// exp(A), column by column into sink(i, column i).  The squaring path (kind 13, rare) parks
// the scaled approximant in the lane's global scratch slot `scr` (two D x D column-major
// tiles) and squares it there element by element, so that it adds no live registers to the
// common path.  FENCE: pin every column and keep the scheduler from overlapping them (register
// discipline at D = 4; at D <= 3 the columns and sectors may interleave for ILP).
// mu: the diagonal shift (sm_regime): chosen here and returned (choose), or the nominal's (an
// eps-variant); the columns are those of E~ = exp(A - i mu I).
template <int D, bool FENCE, bool SHIFT, class Sink>
__device__ __forceinline__ void walk_expm(SM<D> &A, cd *scr, double &mu, bool choose, Sink &&sink) {
    int s = 0;
    const int kind = sm_regime<D, SHIFT>(A, s, mu, choose);
    if (kind == 0) {  // isdiag(A): exp of the diagonal (Julia's fast path)
#pragma unroll
        for (int i = 0; i < D; ++i) {
            cd x[D];
            const double a = A.d[i] - mu;  // (exact for mu = 0)
            const double sn = sin(a), cn = cos(a);  // exp(0) (cos, sin), as the row-group path
#pragma unroll
            for (int j = 0; j < D; ++j) x[j] = (j == i) ? cmake(cn, sn) : czero();
            if (FENCE) pin<D>(x);
            sink(i, x);
        }
        return;
    }
    SM<D> A2, A3;
    sm_cube<D>(A, A2, A3);
    if (kind != 13) {
        const int nst = kind == 3 ? 1 : kind == 4 ? 2 : 3;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            cd x[D];
            sm_taylor_col<D>(nst, i, A, A2, A3, x);
            sink(i, x);
            if (FENCE) __builtin_amdgcn_sched_barrier(0);
        }
        return;
    }
    cd *T = scr, *R = scr + D * D;
#pragma unroll
    for (int i = 0; i < D; ++i) {  // (unrolled: register arrays are only ever indexed by constants)
        cd x[D];
        sm_taylor_col_hi<D>(i, A, A2, A3, x);
#pragma unroll
        for (int j = 0; j < D; ++j) T[i * D + j] = x[j];
    }
#pragma unroll 1
    for (int r = 0; r < s; ++r) {  // T <- T T, column-major tiles
        __threadfence_block();
#pragma unroll 1
        for (int i = 0; i < D; ++i) {
#pragma unroll 1
            for (int j = 0; j < D; ++j) {
                cd c = czero();
#pragma unroll
                for (int m = 0; m < D; ++m) cmac(c, T[m * D + j], T[i * D + m]);
                R[i * D + j] = c;
            }
        }
        cd *t = T;
        T = R;
        R = t;
    }
    __threadfence_block();
#pragma unroll
    for (int i = 0; i < D; ++i) {
        cd x[D];
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = T[i * D + j];
        if (FENCE) pin<D>(x);
        sink(i, x);
    }
}

// Problem data every lane reads at the same address (term tables, the sector's operators) is
// read through the constant address space: scalar loads into SGPRs from the scalar cache, off
// the vector-memory counter (through a flat pointer the compiler cannot rule out that the
// kernel's own stores alias them and issues per-lane vector loads, a dependent chain of them per
// term -- the round-3 first cut spent 74 % of k_walk_fwd<2>'s wave cycles waiting on it).
template <class T>
using cptr = const __attribute__((address_space(4))) T *;
template <class T>
__device__ __forceinline__ cptr<T> as_constant(const T *p) {
    return (cptr<T>)(p);
}
// field-wise copies out of the constant address space (a reference cannot bind across spaces)
__device__ __forceinline__ cd cload(cptr<cd> p, size_t i) { return cmake(p[i].re, p[i].im); }
__device__ __forceinline__ Term tload(cptr<Term> p, int i) {
    Term t;
    t.op = p[i].op;
    t.var = p[i].var;
    t.index = p[i].index;
    t.func = p[i].func;
    t.a = p[i].a;
    t.b = p[i].b;
    t.sre = p[i].sre;
    t.sim = p[i].sim;
    return t;
}
__device__ __forceinline__ Pert pload(cptr<VSpec> p, int i) {
    Pert q;
    q.var = p[i].pert.var;
    q.index = p[i].pert.index;
    q.delta = p[i].pert.delta;
    return q;
}

// The step's controls x[:, k] (np <= 2) and x_add (na <= 2) in registers:
// the next step's controls are loaded one step ahead, so the build never waits on memory.
struct WalkX {  // named registers (an array picked by index would be demoted to scratch)
    double k0, k1;  // x[:, k]  (np <= kWalkMaxNpA = 2)
    double a0, a1;  // x_add    (na <= 2)
    __device__ __forceinline__ double xk(int i) const { return i == 0 ? k0 : k1; }
    __device__ __forceinline__ double xa(int i) const { return i == 0 ? a0 : a1; }
};
struct X2 {
    double v0, v1;
};
// Unconditional loads (the second one clamped into the vector): a load under a branch leaves the
// compiler without a static count of the outstanding vector-memory operations, and it then waits
// with vmcnt(0) -- for every store of the step too -- before the prefetched value is used.
// xs: consecutive values of this lane's row of x
__device__ __forceinline__ X2 walk_load_x(int n, const double *xs) {  // n (uniform) <= 2 values
    X2 r;
    const double a = xs[0], b = xs[n > 1 ? 1 : 0];
    r.v0 = n > 0 ? a : 0.0;
    r.v1 = n > 1 ? b : 0.0;
    return r;
}
__device__ __forceinline__ void walk_set_xk(WalkX &X, const X2 &r) {
    X.k0 = r.v0;
    X.k1 = r.v1;
}
__device__ __forceinline__ void walk_set_xa(WalkX &X, const X2 &r) {
    X.a0 = r.v0;
    X.a1 = r.v1;
}

// term_coef (grape_kernels.hpp) with the variable read from registers
__device__ __forceinline__ cd walk_coef(const Term &t, int nt1, const WalkX &X, const Pert &pp, TrigCache &tc) {
    double v = 1.0;
    if (t.var == VAR_X) v = X.xk(t.index);
    else if (t.var == VAR_XADD) v = X.xa(t.index);
    else if (t.var == VAR_TSTEP) v = (double)nt1;
    if (t.var == pp.var && t.index == pp.index) v = v + pp.delta;
    const double arg = t.a * v + t.b;  // built with -ffp-contract=off: no fusion, like Julia
    double fr = 1.0, fi = 0.0;
    if (t.func == FN_LINEAR) fr = arg;
    else if (t.func == FN_COS || t.func == FN_SIN || t.func == FN_CIS) {
        tc.at(arg);
        if (t.func == FN_COS) fr = tc.c;
        else if (t.func == FN_SIN) fr = tc.s;
        else {
            fr = tc.c;
            fi = tc.s;
        }
    }
    return cmul(cmake(t.sre, t.sim), cmake(fr, fi));
}

// A_w += g H_w-term for the NS sectors of this lane (compressed; diagonal as the imaginary part
// of the same complex MAC)
template <int D, int NS>
__device__ __forceinline__ void walk_add_term(const DevProblem &P, cptr<cd> ops, int op_index, cd g, SM<D> (&A)[NS]) {
#pragma unroll
    for (int w = 0; w < NS; ++w) {
        const cptr<cd> op = ops + (size_t)w * P.sec_ops + (size_t)op_index * D * D;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const cd o = cload(op, j * D + j);
            A[w].d[j] = fma(g.im, o.re, fma(g.re, o.im, A[w].d[j]));
#pragma unroll
            for (int k = j + 1; k < D; ++k) cmac(A[w].u[uix(D, j, k)], g, cload(op, j * D + k));
        }
    }
}

// A_w = -i dt H_w(x_k perturbed by pp) for the NS sectors w of this lane, compressed: the
// builder of ItemBuilder with each sector's row-major operators, term by term in order (the same
// cmac operand roles).  The term coefficients (the trig of the controls) are computed once for all
// NS sectors.  err >= 0 adds errval Herror_err (perturbed by pp too) after H0's terms, as
// ItemBuilder<D, true> does (UnitaryCalculations.jl:67-68, 71-72, 77-78).
template <int D, int NS>
__device__ __forceinline__ void walk_build(const DevProblem &P, cptr<cd> ops, const WalkX &X, int nt1, const Pert &pp,
                                           SM<D> (&A)[NS], int err = -1, double errval = 0.0) {
#pragma unroll
    for (int w = 0; w < NS; ++w) {
#pragma unroll
        for (int j = 0; j < D; ++j) A[w].d[j] = 0.0;
#pragma unroll
        for (int t = 0; t < SM<D>::NU; ++t) A[w].u[t] = czero();
    }
    TrigCache tc;
    const cptr<Term> terms = as_constant(P.h0);
#pragma unroll 1
    for (int t = 0; t < P.n_h0; ++t) {
        const Term tm = tload(terms, t);
        const cd c = walk_coef(tm, nt1, X, pp, tc);
        walk_add_term<D, NS>(P, ops, tm.op, cmake(P.dt * c.im, -(P.dt * c.re)), A);  // -i dt c
    }
    if (err >= 0) {  // (wave-uniform)
        const cptr<int> off = as_constant(P.err_off);
        const int o0 = off[err], o1 = off[err + 1];
        const cptr<Term> et = as_constant(P.err);
#pragma unroll 1
        for (int t = o0; t < o1; ++t) {
            const Term tm = tload(et, t);
            const cd c = cscale(errval, walk_coef(tm, nt1, X, pp, tc));
            walk_add_term<D, NS>(P, ops, tm.op, cmake(P.dt * c.im, -(P.dt * c.re)), A);
        }
    }
}

// A lane's D x D matrix: registers, or (D = 4, where registers run out) its private LDS slot,
// row-major, 17 complex apart so that the 16-B accesses of 16 lanes hit 64 distinct banks.
template <int D, bool LDS>
struct MStore;
template <int D>
struct MStore<D, false> {
    cd e[D][D];
    __device__ __forceinline__ cd at(int j, int k) const { return e[j][k]; }
    __device__ __forceinline__ void set(int j, int k, cd v) { e[j][k] = v; }
    __device__ __forceinline__ const MStore &opaque() const { return *this; }
};
using lds_cd = __attribute__((address_space(3))) cd;  // typed LDS pointer: ds_read / ds_write, never flat
template <int D>
struct MStore<D, true> {
    static constexpr int kStride = D * D + 1;
    lds_cd *p;
    __device__ __forceinline__ cd at(int j, int k) const { return cmake(p[j * D + k].re, p[j * D + k].im); }
    __device__ __forceinline__ void set(int j, int k, cd v) {
        p[j * D + k].re = v.re;
        p[j * D + k].im = v.im;
    }
    __device__ __forceinline__ static lds_cd *slot(cd *lds_base) {  // this lane's slot
        return (lds_cd *)(lds_base) + threadIdx.x * kStride;
    }
    // a copy whose address the compiler cannot see through: its loads stay where they are
    // written (no hoisting of 64 VGPRs of LDS reads out of a loop or across an exponential)
    __device__ __forceinline__ MStore opaque() const {
        MStore o{p};
        asm volatile("" : "+v"(o.p));
        return o;
    }
};

// Launch geometry: one lane per (chunk c, evaluation be) -- the evaluation fastest, so that a
// wave's stores of its F_dx terms (B.sec_part, evaluation-fastest) are contiguous -- and group of NS sectors (w0 = NS * blockIdx.y);
// sub-evaluation of sector w: be * nsec + w.  Lanes past the end (ok = false) run the walk on
// clamped indices and store nothing, so that every loop in the walks has a wave-uniform trip
// count (scalar loads of the term tables).
struct WalkLane {
    int w0, be, c, nbe;  // nbe: evaluations of the launch (the stride of B.sec_part)
    long slot;           // the lane's scratch slot (NS consecutive pairs of D x D tiles)
    bool ok;
};
// The workgroup's place in the class's launch grid: the hardware block, or (pair kernels, two
// sector classes in one launch for latency-bound calls) a block of one class's part of the grid.
struct VBlock {
    int x, y, gx;  // blockIdx.x, blockIdx.y, gridDim.x of the class's own grid
};
__device__ __forceinline__ VBlock hw_block() { return VBlock{(int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x}; }
template <int NS>
__device__ __forceinline__ WalkLane walk_lane(const DevProblem &P, const DevBatch &B, const VBlock &vb) {
    WalkLane L;
    const int ns = P.nsec > 1 ? P.nsec : 1;
    L.nbe = B.nb / ns;
    const long per = (long)L.nbe * P.nchunks;
    const long g = (long)vb.x * kWalkBlock + threadIdx.x;
    L.w0 = vb.y * NS;
    L.ok = g < per;
    const long gg = L.ok ? g : 0;
    L.c = (int)(gg / L.nbe);
    L.be = (int)(gg - (long)L.c * L.nbe);
    // own scratch slot for every lane, past-the-end ones included (they walk lane 0's inputs)
    const long per_pad = (per + kWalkBlock - 1) / kWalkBlock * kWalkBlock;
    L.slot = (long)vb.y * per_pad + g;
    return L;
}

// The build's knobs of the walks: plain numbers (waves per SIMD for __launch_bounds__), A/B'd from one tree
// with -D (scripts/build_variants.py), and the three code paths bench.py's FLOP model reads from the build's
// defines.  What was measured with them is in DESIGN.md 9 and 10.
#ifndef GRAPE_WALK_F4_WAVES  // k_walk_fwd<4>
#define GRAPE_WALK_F4_WAVES 2
#endif
#ifndef GRAPE_WALK_F3_WAVES  // k_walk_fwd<3>
#define GRAPE_WALK_F3_WAVES 2
#endif
#ifndef GRAPE_WALK_F22_WAVES  // k_walk_fwd<2, 2>
#define GRAPE_WALK_F22_WAVES 3
#endif
#ifndef GRAPE_WALK_G4_WAVES  // k_walk_grad<4> (recomputed propagators)
#define GRAPE_WALK_G4_WAVES 1
#endif
#ifndef GRAPE_WALK_G4S_WAVES  // k_walk_grad<4> with stored propagators
#define GRAPE_WALK_G4S_WAVES 1
#endif
#ifndef GRAPE_WALK_G3_WAVES  // k_walk_grad<3, 1> (recomputed propagators)
#define GRAPE_WALK_G3_WAVES 2
#endif
#ifndef GRAPE_WALK_G3S_WAVES  // k_walk_grad<3, 1> with stored propagators
#define GRAPE_WALK_G3S_WAVES 1
#endif
#ifndef GRAPE_WALK_G22_WAVES  // k_walk_grad<2, 2>
#define GRAPE_WALK_G22_WAVES 3
#endif
#ifndef GRAPE_WALK_I21_WAVES  // k_walk_img<2, 1>
#define GRAPE_WALK_I21_WAVES 3
#endif
#ifndef GRAPE_WALK_I22_WAVES  // k_walk_img<2, 2>
#define GRAPE_WALK_I22_WAVES 2
#endif
#ifndef GRAPE_WALK_GAUGE2_WAVES  // phase-covariant chunk walks of 2 levels ...
#define GRAPE_WALK_GAUGE2_WAVES 4
#endif
#ifndef GRAPE_WALK_GAUGE3_WAVES  // ... of 3 ...
#define GRAPE_WALK_GAUGE3_WAVES 3
#endif
#ifndef GRAPE_WALK_GAUGE4_WAVES  // ... and of 4
#define GRAPE_WALK_GAUGE4_WAVES 2
#endif
#ifndef GRAPE_WALK_FWD_M_WAVES  // the merged forward walk (120 VGPRs with E~ in SGPRs)
#define GRAPE_WALK_FWD_M_WAVES 4
#endif
#ifndef GRAPE_WALK_MERGED_WAVES  // the merged matrix gradient walk (222 VGPRs with E~ in registers)
#define GRAPE_WALK_MERGED_WAVES 2
#endif
#ifndef GRAPE_WALK_R1_WAVES  // the merged rank-one gradient walk (108 VGPRs with E~ in SGPRs)
#define GRAPE_WALK_R1_WAVES 3
#endif
#ifndef GRAPE_WALK_WIDE_FWD_WAVES  // the wide forward walk (10 VGPRs of state)
#define GRAPE_WALK_WIDE_FWD_WAVES 4
#endif
#ifndef GRAPE_WALK_WIDE_GRAD_WAVES  // the wide gradient walk
#define GRAPE_WALK_WIDE_GRAD_WAVES 4
#endif
#ifndef GRAPE_WALK_WSUM_LAB_WAVES  // k_walk_wsum_lab
#define GRAPE_WALK_WSUM_LAB_WAVES 2
#endif
#ifndef GRAPE_WALK_ERR_LAB_WAVES  // k_walk_err_lab at 2 and 3 levels
#define GRAPE_WALK_ERR_LAB_WAVES 2
#endif
#ifndef GRAPE_WALK_ERR_LAB4_WAVES  // k_walk_err_lab<4>: four 4 x 4 complex matrices live (256 VGPRs) at the peak
#define GRAPE_WALK_ERR_LAB4_WAVES 2
#endif
#ifndef GRAPE_WALK_TWIN_SUM  // merged gradient walk, twin class B: one summed state for both sectors
#define GRAPE_WALK_TWIN_SUM 1
#endif
#ifndef GRAPE_WALK_LADDER_CONTR  // ladder classes: the contraction grouped by charge difference
#define GRAPE_WALK_LADDER_CONTR 1
#endif
#ifndef GRAPE_WIDE_TILE_FAST  // wide walks: full workgroup and full tile move x and F_dx by a uniform stride
#define GRAPE_WIDE_TILE_FAST 1
#endif
#ifndef GRAPE_WIDE_STEP_FRAME  // wide forward walk, ladder charges: chi = D_k^dag psi walked through E~ itself
#define GRAPE_WIDE_STEP_FRAME 1
#endif
template <int D, int NS>
struct WalkCfg {
    static constexpr bool FENCE = D >= 4;        // per-column scheduling fences (register discipline)
    static constexpr bool X_LDS = D >= 4 && NS == 1;  // k_walk_grad: X / Y in the lane's LDS slot, E in registers
    static constexpr int WAVES_FWD = D <= 2 ? (NS == 1 ? 4 : NS == 2 ? GRAPE_WALK_F22_WAVES : 3)
                                   : D == 3 ? GRAPE_WALK_F3_WAVES : GRAPE_WALK_F4_WAVES;
    static constexpr int WAVES_GRAD = D <= 2 ? (NS == 1 ? 4 : NS == 2 ? GRAPE_WALK_G22_WAVES : 2)
                                    : D == 3 ? (NS == 1 ? GRAPE_WALK_G3_WAVES : 1) : GRAPE_WALK_G4_WAVES;
    static constexpr int WAVES_GRAD_STORED = D <= 2 ? (NS == 1 ? 3 : 2) : D == 3 ? GRAPE_WALK_G3S_WAVES : GRAPE_WALK_G4S_WAVES;
    static constexpr int WAVES_IMG = D <= 2 ? (NS == 1 ? GRAPE_WALK_I21_WAVES : GRAPE_WALK_I22_WAVES) : 1;  // k_walk_img
    static constexpr bool IMG_LDS = D >= 4;      // k_walk_img: eps2 propagators in LDS
    // the diagonal shift + Taylor 9 (sm_regime) where the Taylor-12 columns dominate; the 2-level classes
    // (Taylor 6 at C2) keep the unshifted walk bitwise
    static constexpr bool SHIFT = D >= 3;
    // phase-covariant classes (GAUGE): E~, E and the walk state only -- no exponential per step
    static constexpr int WAVES_GAUGE = D <= 2 ? (NS >= 3 ? 2 : GRAPE_WALK_GAUGE2_WAVES)
                                              : D == 3 ? GRAPE_WALK_GAUGE3_WAVES : GRAPE_WALK_GAUGE4_WAVES;
};

// The chunk's phase: sum of the steps' diagonal shifts (sm_regime), TwoSum-compensated; the chunk
// total is e^{i phi} Q~ with Q~ the product of the shifted propagators.
struct WalkPhase {
    double hi = 0.0, lo = 0.0;
    __device__ __forceinline__ void add(double m) {  // (adding 0 is exact: steps past N_t)
        const double t = hi + m, bp = t - hi;
        lo += (hi - (t - bp)) + (m - bp);
        hi = t;
    }
};
template <int D>
__device__ __forceinline__ void walk_phase(const WalkPhase &ph, cd (&Q)[D][D]) {
    const double phi = ph.hi + ph.lo;
    if (phi == 0.0) return;  // (no shift: Q~ is the total)
    double sn, cn;
    sincos(phi, &sn, &cn);
#pragma unroll
    for (int j = 0; j < D; ++j) {
#pragma unroll
        for (int i = 0; i < D; ++i) Q[j][i] = cmul(cmake(cn, sn), Q[j][i]);
    }
}
// Stored propagators (B.Ew): per (step, sector) the D*D elements of E~ and, as element D*D, the
// shift mu (real part), each element one coalesced row over the launch's lanes.
template <int D>
constexpr int kEwStride = D * D + 1;

// Two D x D products that more than one family's chunk start takes (the merged gradient walks and
// k_walk_err_lab; k_walk_err_grad and k_walk_err_lab)
// C = A Bm, row-major tiles
template <int D>
__device__ __forceinline__ void walk_mm(const cd (&A)[D * D], const cd (&Bm)[D * D], cd (&C)[D * D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            cd c = czero();
#pragma unroll
            for (int m = 0; m < D; ++m) cmac(c, A[i * D + m], Bm[m * D + j]);
            C[i * D + j] = c;
        }
    }
}
// X = Carry_c M_ww Carry_c^dag of sector w (walk_grad_body's arithmetic)
template <int D>
__device__ __forceinline__ void merged_xinit(const cd *Cr, const cd *Mw, cd (&X)[D][D]) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
        cd r[D];
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
            X[i][j] = acc;
        }
    }
}

}  // namespace grape
