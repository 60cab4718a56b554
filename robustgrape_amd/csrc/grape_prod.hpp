// grape_prod.hpp -- product coefficients (grape.h GRAPE_OP_FACTOR) on the stored pipeline of the small-d
// engine: the generator's builder with factor terms, and the two kernels that build a generator from
// terms with it.
//
//   k_expm_prod       k_expm's body (grape_kernels.hpp expm_item_body) over ProdItemBuilder
//   k_expm_grad_prod  k_expm_grad's body (expm_grad_item_body) over ProdItemBuilder
//
// Every other kernel of the stored pipeline reads parked slots (k_expm_high, k_grad_high) or stored
// propagators (the scans, the heads, k_err_*), so these two are all a plan with factor terms swaps.  They
// take the factor table as a kernel argument of its own.  Compiled in a unit of their own per dimension
// (grape_prod_inst.hip): the units of the plain kernels keep their machine code.
#pragma once
#include "grape_launch.hpp"

namespace grape {

// ItemBuilder with product coefficients: the coefficient of an operator term is term_coef of the term
// times the (real) term_coef of each of its factors.  One TrigCache serves the term and its factors in
// list order, so cos(phi) Hc and sin(phi) Hs with a linear amplitude factor each still share one sincos.
// The perturbation of a variant reaches every factor that reads the perturbed variable (term_coef
// compares var / index itself): x cos x is differenced in both places, as the reference's closure is.
// Register discipline as ItemBuilder: constant-index arrays, value selects, the factor slots unrolled.
template <int D, bool ERR>
struct ProdItemBuilder {
    const DevProblem *P;
    FactorTab F;
    const cd *opsT;  // this item's sector of the column-major basis
    const double *xk, *xadd;
    int i, nt1;
    VSpec vs;
    bool valid;
    cd c0[kCachedTerms], ce[kCachedTerms];  // products pre-scaled by -i dt (and errval)
    int o0, ne_t;

    // -i dt c
    __device__ __forceinline__ cd gen(cd c) const { return cmake(P->dt * c.im, -(P->dt * c.re)); }

    // term t of a list times its factors (fac: the list's factor slots)
    __device__ __forceinline__ cd coef(const Term *terms, const Term *fac, int t, TrigCache &tc) const {
        cd c = term_coef(terms[t], nt1, xk, xadd, vs.pert, tc);
#pragma unroll
        for (int j = 0; j < kMaxFactors; ++j) {
            const Term f = fac[t * kMaxFactors + j];
            if (f.op) c = cscale(term_coef(f, nt1, xk, xadd, vs.pert, tc).re, c);  // launch-uniform branch
        }
        return c;
    }

    __device__ __forceinline__ ProdItemBuilder(const DevProblem *P_, const FactorTab &F_, const double *xk_,
                                               const double *xadd_, int i_, int nt1_, const VSpec &vs_, bool valid_,
                                               int sector = 0)
        : P(P_), F(F_), opsT(P_->opsT + (size_t)sector * P_->sec_ops), xk(xk_), xadd(xadd_), i(i_), nt1(nt1_),
          vs(vs_), valid(valid_), o0(0), ne_t(0) {
        TrigCache tc;
#pragma unroll
        for (int t = 0; t < kCachedTerms; ++t) c0[t] = (t < P->n_h0) ? gen(coef(P->h0, F.h0, t, tc)) : czero();
        if (ERR && vs.err >= 0) {
            o0 = P->err_off[vs.err];
            ne_t = P->err_off[vs.err + 1] - o0;
#pragma unroll
            for (int t = 0; t < kCachedTerms; ++t)
                ce[t] = (t < ne_t) ? gen(cscale(vs.errval, coef(P->err + o0, F.err + (size_t)o0 * kMaxFactors, t, tc)))
                                   : czero();
        }
    }

    __device__ __forceinline__ void accumulate(const Term *terms, const Term *fac, int n,
                                               const cd (&cache)[kCachedTerms], double sc, cd (&h)[D]) const {
#pragma unroll
        for (int t = 0; t < kCachedTerms; ++t) {
            if (t < n) {
                const cd *op = opsT + (size_t)terms[t].op * D * D + i * D;
#pragma unroll
                for (int j = 0; j < D; ++j) cmac(h[j], cache[t], op[j]);
            }
        }
        for (int t = kCachedTerms; t < n; ++t) {  // more operator terms than cached: each with a cache of its own
            TrigCache tc;
            const cd c = gen(cscale(sc, coef(terms, fac, t, tc)));
            const cd *op = opsT + (size_t)terms[t].op * D * D + i * D;
#pragma unroll
            for (int j = 0; j < D; ++j) cmac(h[j], c, op[j]);
        }
    }

    // column i of A = -i dt (H0 [+ errval Herror])
    __device__ __forceinline__ void operator()(cd (&a)[D]) const {
#pragma unroll
        for (int j = 0; j < D; ++j) a[j] = czero();
        accumulate(P->h0, F.h0, P->n_h0, c0, 1.0, a);
        if (ERR && vs.err >= 0) accumulate(P->err + o0, F.err + (size_t)o0 * kMaxFactors, ne_t, ce, vs.errval, a);
        if (!valid) {
#pragma unroll
            for (int j = 0; j < D; ++j) a[j] = czero();
        }
    }
};

template <int D, bool ERR>
__global__ __launch_bounds__(64, (D <= 9 ? GRAPE_EXPM_WAVES_D9 : 2)) void k_expm_prod(DevProblem P, DevBatch B,
                                                                                      FactorTab F) {
    expm_item_body<D, ERR>(P, B, [&](const double *xk, const double *xadd, int i, int nt1, const VSpec &vs, bool valid,
                                     int sector) { return ProdItemBuilder<D, ERR>(&P, F, xk, xadd, i, nt1, vs, valid, sector); });
}

template <int D>
__global__ __launch_bounds__(64, (D <= 9 ? GRAPE_EXPM_GRAD_WAVES : 2)) void k_expm_grad_prod(DevProblem P, DevBatch B,
                                                                                             FactorTab F) {
    expm_grad_item_body<D>(P, B, [&](const double *xk, const double *xadd, int i, int nt1, const VSpec &vs, bool valid,
                                     int sector) { return ProdItemBuilder<D, false>(&P, F, xk, xadd, i, nt1, vs, valid, sector); });
}

}  // namespace grape

namespace grape_host {

// every variant of every (b, k) into B.E (err: the builder with error terms); the launch geometry of k_expm
template <int D>
hipError_t launch_expm_prod(bool err, const DevProblem &P, const DevBatch &B, const grape::FactorTab &F,
                            hipStream_t st) {
    constexpr int GPW = grape::Geo<D>::GPW;
    const long nexp = (long)B.nb * P.Nt * P.nv;
    if (err)
        hipLaunchKernelGGL((grape::k_expm_prod<D, true>), dim3((unsigned)((nexp + GPW - 1) / GPW)), dim3(64),
                           expm_lean_lds<D>(), st, P, B, F);
    else
        hipLaunchKernelGGL((grape::k_expm_prod<D, false>), dim3((unsigned)((nexp + GPW - 1) / GPW)), dim3(64),
                           expm_lean_lds<D>(), st, P, B, F);
    return hipGetLastError();
}

// the eps-variants contracted in place; the launch geometry of k_expm_grad
template <int D>
hipError_t launch_expm_grad_prod(const DevProblem &P, const DevBatch &B, const grape::FactorTab &F, hipStream_t st) {
    constexpr int GPW = grape::Geo<D>::GPW;
    const int nvg = P.np + (P.xadd_dep ? P.na : 0);
    const long ng = (long)B.nb * P.Nt * nvg;
    hipLaunchKernelGGL(grape::k_expm_grad_prod<D>, dim3((unsigned)((ng + GPW - 1) / GPW)), dim3(64), expm_lean_lds<D>(),
                       st, P, B, F);
    return hipGetLastError();
}

}  // namespace grape_host
