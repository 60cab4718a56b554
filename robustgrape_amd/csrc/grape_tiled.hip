// grape_tiled.hip -- the tiled engine's kernels (64 < d <= 128, images in HBM, products tiled
// through LDS on MFMA; building blocks and layouts: grape_tiled.hpp).  The algebra is the dense
// engine's (grape_dense.hip header), one batched launch per product:
//
//   k_tctl      one workgroup per (eval b, step k): |A_k|_1 of A_k = -i dt H(x_b, k), from it the
//               Taylor degree and the squaring count s of the step (nominal AND eps-variants).
//   k_tgen      A_k / 2^s (nominal or one control perturbed) as an image.        UnitaryCalculations.jl:45
//   k_tprod     C = op(L) op(R) for every item of a launch; the operands come from an address
//               functor: the exponential's powers / Horner steps / squarings (ExpPow, ExpStep) or a
//               pipeline stage (PipeAddr: chunk-local prefixes Q_k = E_k Q_{k-1}, carries, U,
//               K = U0^dag U, K^dag W K, M'_c = Carry_c M Carry_c^dag, Y_k^dag = Q_k (Q_{k-1} M'_c)^dag).
//   k_ttop      the initial Paterson-Stockmeyer block of every item.
//   k_ttarget   U0(x_add) and (U0(x_add + eps e_q) - U0) / eps.                  FidelityCalculations.jl:32-40
//   k_thead1/2  tau, F, W K, the target part of F_dx_add; M = G U.               FidelityCalculations.jl:47-76
//   k_tcontract F_dx[p, k] = Re sum conj(Y_k^dag) o (E' - E_k) / eps.            FidelityCalculations.jl:56-65
#include "grape_tiled.hpp"
#include "grape_tiled_api.hpp"

namespace grape_tiled {

namespace {

constexpr grape::Pert kNoPert = {-1, 0, 0.0};

// ---------------------------------------------------------------------------
// products
// ---------------------------------------------------------------------------
template <bool LCT, bool RCT, class Addr>
__global__ __launch_bounds__(NTHREADS) void k_tprod(Geo g, Addr addr) {
    __shared__ double lds[4 * SLAB];
    Ops o;
    if (!addr((int)(blockIdx.x >> 2), o)) return;  // (uniform over the workgroup)
    tile_product<LCT, RCT>(g, o, (int)(blockIdx.x & 3), lds);
}

// A^2 = A A, A^3 = A A^2, A^4 = A^2 A^2 of every item of a slab
struct ExpPow {
    int which;
    ExpSlab X;
    size_t img;
    __device__ bool operator()(int i, Ops &o) const {
        const size_t off = (size_t)i * img;
        o.L = (which == 2 ? X.A2 : X.A) + off;
        o.R = (which == 0 ? X.A : X.A2) + off;
        o.C = (which == 0 ? X.A2 : which == 1 ? X.A3 : X.A4) + off;
        return true;
    }
};

// Launch g of the exponential of every item of a slab: g = 0 .. 3 the Horner step of block j = 3 - g
// (x <- B_j + A^4 x; an item of Taylor block count top joins at g = 3 - top, its initial block in B0),
// g = 4 + q squaring q (x <- x x; an item of squaring count s takes the first s).  An item's n-th product
// reads buffer n & 1 and writes the other one, its last product writes `out`: no copies, and an item
// that is finished, or not yet started, costs a workgroup that returns at once.
struct ExpStep {
    int g;
    const int *ctl;
    ExpSlab X;
    double *out;
    size_t img;
    __device__ bool operator()(int i, Ops &o) const {
        const int c = ctl[i], top = c & 3, s = c >> 2;
        int n;
        if (g < 4) {
            if (g < 3 - top) return false;
            n = g - (3 - top);
        } else {
            if (g - 4 >= s) return false;
            n = top + 1 + (g - 4);
        }
        const bool last = g == 3 + s;
        const size_t off = (size_t)i * img;
        const double *src = ((n & 1) ? X.B1 : X.B0) + off;
        o.C = last ? out + off : ((n & 1) ? X.B0 : X.B1) + off;
        o.R = src;
        if (g < 4) {
            const int j = 3 - g;
            o.L = X.A4 + off;
            o.X1 = X.A + off;
            o.X2 = X.A2 + off;
            o.X3 = X.A3 + off;
            o.c0 = kInvFact[4 * j];
            o.c1 = kInvFact[4 * j + 1];
            o.c2 = kInvFact[4 * j + 2];
            o.c3 = kInvFact[4 * j + 3];
        } else {
            o.L = src;
        }
        return true;
    }
};

// where the pipeline's matrices live (aliases instead of copies: a chunk's first prefix is the step's
// propagator, the first carry is a prefix, M'_0 is M)
struct Ctx {
    int Nt, Nc, Lc, na;
    size_t img;
    double *E, *Q, *Carry, *Tm, *Mc, *U, *M, *WK, *T, *U0, *K, *Ts, *Yd;
    __device__ double *qimg(int b, int k) const {
        return ((k % Lc) == 0 ? E : Q) + ((size_t)b * Nt + k) * img;
    }
    __device__ int kend(int c) const { return min((c + 1) * Lc, Nt) - 1; }
    __device__ double *carry(int b, int c) const {  // c >= 1
        return c == 1 ? qimg(b, kend(0)) : Carry + ((size_t)b * Nc + c) * img;
    }
    __device__ double *uimg(int b) const { return Nc == 1 ? qimg(b, Nt - 1) : U + (size_t)b * img; }
    __device__ double *mcimg(int b, int c) const {
        return c == 0 ? M + (size_t)b * img : Mc + ((size_t)b * Nc + c) * img;
    }
};

enum Stage { ST_SCAN, ST_CARRY, ST_HEADK, ST_HEADT, ST_MC1, ST_MC2, ST_Y1, ST_Y2 };

struct PipeAddr {
    Ctx c;
    int stage;
    int j;   // ST_SCAN: position in the chunk; ST_CARRY: chunk; ST_Y1 / ST_Y2: first step of the slab
    __device__ bool operator()(int i, Ops &o) const {
        switch (stage) {
        case ST_SCAN: {  // item (b, chunk): Q_k = E_k Q_{k-1}, k = chunk Lc + j
            const int b = i / c.Nc, ch = i % c.Nc, k = ch * c.Lc + j;
            if (k >= c.Nt) return false;
            o.L = c.E + ((size_t)b * c.Nt + k) * c.img;
            o.R = c.qimg(b, k - 1);
            o.C = c.Q + ((size_t)b * c.Nt + k) * c.img;
            return true;
        }
        case ST_CARRY: {  // item b: Carry_j = Q_end(j - 1) Carry_{j-1}, j = 2 .. Nc (j = Nc: U)
            o.L = c.qimg(i, c.kend(j - 1));
            o.R = c.carry(i, j - 1);
            o.C = j == c.Nc ? c.U + (size_t)i * c.img : c.Carry + ((size_t)i * c.Nc + j) * c.img;
            return true;
        }
        case ST_HEADK: {  // item (b, v): K = U0^dag U, Kd_q = dU0_q^dag U
            const int b = i / (1 + c.na);
            o.L = c.U0 + (size_t)i * c.img;
            o.R = c.uimg(b);
            o.C = c.K + (size_t)i * c.img;
            return true;
        }
        case ST_HEADT: {  // item b: K^dag (W K)
            o.L = c.K + (size_t)i * (1 + c.na) * c.img;
            o.R = c.WK + (size_t)i * c.img;
            o.C = c.T + (size_t)i * c.img;
            return true;
        }
        case ST_MC1:
        case ST_MC2: {  // item (b, chunk >= 1): Carry M, then (Carry M) Carry^dag
            const int b = i / c.Nc, ch = i % c.Nc;
            if (ch == 0) return false;
            double *tm = c.Tm + (size_t)i * c.img;
            if (stage == ST_MC1) {
                o.L = c.carry(b, ch);
                o.R = c.M + (size_t)b * c.img;
                o.C = tm;
            } else {
                o.L = tm;
                o.R = c.carry(b, ch);
                o.C = c.Mc + (size_t)i * c.img;
            }
            return true;
        }
        default: {  // ST_Y1 / ST_Y2, item = step j + i of the pass: T = Q_{k-1} M'_c, Y^dag = Q_k T^dag
            const int step = j + i, b = step / c.Nt, k = step % c.Nt, ch = k / c.Lc;
            const bool first = k == ch * c.Lc;
            double *ts = c.Ts + (size_t)i * c.img;
            if (stage == ST_Y1) {
                if (first) return false;  // (Q_{k-1} is the carry: T is M'_c itself)
                o.L = c.qimg(b, k - 1);
                o.R = c.mcimg(b, ch);
                o.C = ts;
            } else {
                o.L = c.qimg(b, k);
                o.R = first ? c.mcimg(b, ch) : ts;
                o.C = c.Yd + (size_t)i * c.img;
            }
            return true;
        }
        }
    }
};

template <bool LCT, bool RCT, class Addr>
void launch_prod(const Geo &g, const Addr &a, int items, hipStream_t st) {
    if (items <= 0) return;
    hipLaunchKernelGGL((k_tprod<LCT, RCT, Addr>), dim3((unsigned)items * 4u), dim3(NTHREADS), 0, st, g, a);
}

// ---------------------------------------------------------------------------
// generators, norms, the initial block
// ---------------------------------------------------------------------------
// -i dt c_t of every H0 term of step k into LDS (one variable perturbed)
__device__ __forceinline__ void stage_h0_coefs(const grape::DevProblem &P, const double *xb, int k,
                                               const grape::Pert &pp, double *gre, double *gim, int *gop) {
    const double *xk = xb + (size_t)k * P.np;
    const double *xadd = xb + (size_t)P.np * P.Nt;
    for (int t = threadIdx.x; t < P.n_h0; t += blockDim.x) {
        const Term tm = P.h0[t];
        const cd c = grape::term_coef(tm, k + 1, xk, xadd, pp);
        gre[t] = P.dt * c.im;  // -i dt c
        gim[t] = -(P.dt * c.re);
        gop[t] = tm.op;
    }
    __syncthreads();
}
// sum_t g_t OP_t at image offset a (the dense engine's hm_cmac_img order)
__device__ __forceinline__ void sum_terms(const double *opimg, size_t img, size_t plane, size_t a, int n,
                                          const double *gre, const double *gim, const int *gop, double &re,
                                          double &im) {
    re = 0.0;
    im = 0.0;
    for (int t = 0; t < n; ++t) {
        const double *op = opimg + (size_t)gop[t] * img;
        const double orr = op[a], oi = op[plane + a];
        re = fma(gre[t], orr, re);
        re = fma(-gim[t], oi, re);
        im = fma(gre[t], oi, im);
        im = fma(gim[t], orr, im);
    }
}

// |A|_1 of every item (one workgroup each, thread c sums column c) -> ctl, the pass's largest s, and
// (mstats) Julia's degree histogram.  raw: A is the image raw[item]; else the nominal generator of step item.
__global__ __launch_bounds__(128) void k_tctl(TiledProblem TP, const double *x, const double *raw, int *ctl,
                                               int *smax, int *mstats) {
    __shared__ double gre[kMaxTerms], gim[kMaxTerms], red[128];
    __shared__ int gop[kMaxTerms];
    const grape::DevProblem &P = TP.P;
    const int item = blockIdx.x, Pd = TP.Pd, c = threadIdx.x;
    const size_t plane = (size_t)Pd * Pd, img = 2 * plane;
    if (!raw) stage_h0_coefs(P, x + (size_t)(item / P.Nt) * P.nx, item % P.Nt, kNoPert, gre, gim, gop);
    double cs = 0.0;
    if (c < P.D)
        for (int i = 0; i < P.D; ++i) {
            const size_t a = (size_t)i * Pd + c;
            double re, im;
            if (raw) {
                re = raw[(size_t)item * img + a];
                im = raw[(size_t)item * img + plane + a];
            } else {
                sum_terms(TP.opimg, img, plane, a, P.n_h0, gre, gim, gop, re, im);
            }
            cs += hypot(re, im);
        }
    const double nA = wg_max(cs, red);
    if (threadIdx.x == 0) {
        const int w = make_ctl(nA);
        ctl[item] = w;
        atomicMax(smax, w >> 2);
        if (mstats) atomicAdd(mstats + julia_m_index(nA), 1);
    }
}

// A / 2^s of every item of a slab (item i = step s0 + i of the pass, one variable perturbed; or the raw
// image s0 + i), s from the step's ctl word: an eps-variant is scaled -- and later expanded and squared --
// exactly as its nominal, so that (E' - E) / eps never sees the difference of two roundings.
__global__ __launch_bounds__(NTHREADS) void k_tgen(TiledProblem TP, const double *x, const double *raw, int s0,
                                                    grape::Pert pp, const int *ctl, double *A) {
    __shared__ double gre[kMaxTerms], gim[kMaxTerms];
    __shared__ int gop[kMaxTerms];
    const grape::DevProblem &P = TP.P;
    const int i = blockIdx.x, step = s0 + i, Pd = TP.Pd;
    const size_t plane = (size_t)Pd * Pd, img = 2 * plane;
    if (!raw) stage_h0_coefs(P, x + (size_t)(step / P.Nt) * P.nx, step % P.Nt, pp, gre, gim, gop);
    const double sc = ldexp(1.0, -(ctl[step] >> 2));
    double *dst = A + (size_t)i * img;
    for (size_t a = threadIdx.x; a < plane; a += NTHREADS) {
        double re, im;
        if (raw) {
            re = raw[(size_t)step * img + a];
            im = raw[(size_t)step * img + plane + a];
        } else {
            sum_terms(TP.opimg, img, plane, a, P.n_h0, gre, gim, gop, re, im);
        }
        dst[a] = re * sc;
        dst[plane + a] = im * sc;
    }
}

// B0 = c_{m-4} I + c_{m-3} A + c_{m-2} A^2 + c_{m-1} A^3 + c_m A^4, m = 4 (top + 2)
__global__ __launch_bounds__(NTHREADS) void k_ttop(Geo g, ExpSlab X, const int *ctl) {
    const int i = blockIdx.x, b = 4 * ((ctl[i] & 3) + 1);
    const size_t plane = (size_t)g.P * g.P, off = (size_t)i * 2 * plane;
    const double c0 = kInvFact[b], c1 = kInvFact[b + 1], c2 = kInvFact[b + 2], c3 = kInvFact[b + 3],
                 c4 = kInvFact[b + 4];
    for (size_t a = threadIdx.x; a < plane; a += NTHREADS) {
        const int row = (int)(a / g.P), col = (int)(a % g.P);
        double re = (row == col && row < g.d) ? c0 : 0.0, im = 0.0;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const size_t e = off + pl * plane + a;
            double &v = pl ? im : re;
            v = fma(c1, X.A[e], v);
            v = fma(c2, X.A2[e], v);
            v = fma(c3, X.A3[e], v);
            v = fma(c4, X.A4[e], v);
        }
        X.B0[off + a] = re;
        X.B0[off + plane + a] = im;
    }
}

// the exponentials of the n items whose A / 2^s are in X.A: powers, initial block, Horner steps, squarings
void launch_exp_steps(const Geo &g, const ExpSlab &X, const int *ctl, int n, double *out, int smax,
                      hipStream_t st) {
    const size_t img = 2 * (size_t)g.P * g.P;
    for (int which = 0; which < 3; ++which) launch_prod<false, false>(g, ExpPow{which, X, img}, n, st);
    hipLaunchKernelGGL(k_ttop, dim3((unsigned)n), dim3(NTHREADS), 0, st, g, X, ctl);
    for (int s = 0; s < 4 + smax; ++s) launch_prod<false, false>(g, ExpStep{s, ctl, X, out, img}, n, st);
}

// ---------------------------------------------------------------------------
// head
// ---------------------------------------------------------------------------
// item (b, v): v = 0 the target U0(x_add), v = 1 + q its difference (U0(x_add + eps e_q) - U0) / eps
__global__ __launch_bounds__(NTHREADS) void k_ttarget(TiledProblem TP, const double *x, double *U0) {
    __shared__ double c0r[kMaxTerms], c0i[kMaxTerms], c1r[kMaxTerms], c1i[kMaxTerms];
    __shared__ int gop[kMaxTerms];
    const grape::DevProblem &P = TP.P;
    const int item = blockIdx.x, b = item / (1 + P.na), v = item % (1 + P.na), Pd = TP.Pd;
    const size_t plane = (size_t)Pd * Pd, img = 2 * plane;
    const double *xadd = x + (size_t)b * P.nx + (size_t)P.np * P.Nt;
    for (int t = threadIdx.x; t < P.n_tgt; t += NTHREADS) {
        const Term tm = P.tgt[t];
        const cd c0 = grape::term_coef(tm, 1, xadd, xadd, kNoPert);
        c0r[t] = c0.re;
        c0i[t] = c0.im;
        gop[t] = tm.op;
        if (v > 0) {
            grape::Pert pq;
            pq.var = grape::VAR_XADD;
            pq.index = v - 1;
            pq.delta = P.eps;
            const cd c1 = grape::term_coef(tm, 1, xadd, xadd, pq);
            c1r[t] = c1.re;
            c1i[t] = c1.im;
        }
    }
    __syncthreads();
    double *dst = U0 + (size_t)item * img;
    for (size_t a = threadIdx.x; a < plane; a += NTHREADS) {
        double re, im;
        sum_terms(TP.opimg, img, plane, a, P.n_tgt, c0r, c0i, gop, re, im);
        if (v > 0) {
            double re1, im1;
            sum_terms(TP.opimg, img, plane, a, P.n_tgt, c1r, c1i, gop, re1, im1);
            re = (re1 - re) * P.inv_eps;
            im = (im1 - im) * P.inv_eps;
        }
        dst[a] = re;
        dst[plane + a] = im;
    }
}

// per evaluation: tau = tr(W K), F, W K, and the target part of F_dx_add     FidelityCalculations.jl:47-54, 67-76
__global__ __launch_bounds__(NTHREADS) void k_thead1(TiledProblem TP, TiledBatch B) {
    __shared__ double red[NTHREADS];
    const grape::DevProblem &P = TP.P;
    const int b = blockIdx.x, Pd = TP.Pd;
    const size_t plane = (size_t)Pd * Pd, img = 2 * plane;
    const double *K = B.K + (size_t)b * (1 + P.na) * img;
    double *WK = B.WK + (size_t)b * img;
    double part = 0.0, tre = 0.0, tim = 0.0;
    for (size_t a = threadIdx.x; a < plane; a += NTHREADS) {
        const int row = (int)(a / Pd), col = (int)(a % Pd);
        const double wr = TP.W[row], pcol = TP.W[col] != 0.0 ? 1.0 : 0.0;
        const double kr = K[a], ki = K[plane + a];
        part += wr * (pcol * (kr * kr + ki * ki));
        if (row == col) {
            tre += wr * kr;
            tim += wr * ki;
        }
        WK[a] = wr * kr;
        WK[plane + a] = wr * ki;
    }
    const double sum_part = wg_sum(part, red);
    const double tau_re = wg_sum(tre, red), tau_im = wg_sum(tim, red);
    if (threadIdx.x == 0) {
        B.F[b] = (sum_part + tau_re * tau_re + tau_im * tau_im) / P.DD;
        B.tau[2 * b] = tau_re;
        B.tau[2 * b + 1] = tau_im;
    }
    for (int q = 0; q < P.na; ++q) {
        const double *Kd = K + (size_t)(1 + q) * img;
        double pr = 0.0, dre = 0.0, dim = 0.0;
        for (size_t a = threadIdx.x; a < plane; a += NTHREADS) {
            const int row = (int)(a / Pd), col = (int)(a % Pd);
            const double wr = TP.W[row], pcol = TP.W[col] != 0.0 ? 1.0 : 0.0;
            pr += wr * (pcol * (Kd[a] * K[a] + Kd[plane + a] * K[plane + a]));
            if (row == col) {
                dre += wr * Kd[a];
                dim += wr * Kd[plane + a];
            }
        }
        const double s1 = wg_sum(pr, red), tr_re = wg_sum(dre, red), tr_im = wg_sum(dim, red);
        if (threadIdx.x == 0)
            B.Fdx[(size_t)b * P.nx + (size_t)P.np * P.Nt + q] =
                (2.0 * s1 + 2.0 * (tau_re * tr_re + tau_im * tr_im)) / P.DD;
    }
}

// M = (2 / DD) (P K^dag W K + conj(tau) W K), T = K^dag (W K)
__global__ __launch_bounds__(NTHREADS) void k_thead2(TiledProblem TP, TiledBatch B) {
    const grape::DevProblem &P = TP.P;
    const int b = blockIdx.y, Pd = TP.Pd;
    const size_t plane = (size_t)Pd * Pd, img = 2 * plane;
    const size_t a = (size_t)blockIdx.x * NTHREADS + threadIdx.x;
    if (a >= plane) return;
    const double tau_re = B.tau[2 * b], tau_im = B.tau[2 * b + 1], sc = 2.0 / P.DD;
    const double prow = TP.W[a / Pd] != 0.0 ? 1.0 : 0.0;
    const double *T = B.T + (size_t)b * img, *WK = B.WK + (size_t)b * img;
    const double wr = WK[a], wi = WK[plane + a];
    const double cr = tau_re * wr + tau_im * wi, ci = tau_re * wi - tau_im * wr;  // conj(tau) W K
    double *M = B.M + (size_t)b * img;
    M[a] = sc * (prow * T[a] + cr);
    M[plane + a] = sc * (prow * T[plane + a] + ci);
}

// F_dx[p, k] = Re tr(Y_k (E' - E_k) / eps) = sum Re(Yd) o Re(dE) + Im(Yd) o Im(dE), Yd = Y_k^dag; item i =
// step s0 + i of the pass
__global__ __launch_bounds__(NTHREADS) void k_tcontract(TiledProblem TP, TiledBatch B, int s0, int p) {
    __shared__ double red[NTHREADS];
    const grape::DevProblem &P = TP.P;
    const int i = blockIdx.x, step = s0 + i;
    const size_t plane = (size_t)TP.Pd * TP.Pd, img = 2 * plane;
    const double *E = B.E + (size_t)step * img, *Ev = B.Ev + (size_t)i * img, *Yd = B.Yd + (size_t)i * img;
    double acc = 0.0;
    for (size_t a = threadIdx.x; a < img; a += NTHREADS) acc += Yd[a] * ((Ev[a] - E[a]) * P.inv_eps);
    const double s = wg_sum(acc, red);
    if (threadIdx.x == 0) B.Fdx[(size_t)(step / P.Nt) * P.nx + (size_t)(step % P.Nt) * P.np + p] = s;
}

Ctx make_ctx(const TiledProblem &TP, const TiledBatch &B) {
    Ctx c;
    c.Nt = TP.P.Nt;
    c.Nc = TP.Nc;
    c.Lc = TP.Lc;
    c.na = TP.P.na;
    c.img = 2 * (size_t)TP.Pd * TP.Pd;
    c.E = B.E;
    c.Q = B.Q;
    c.Carry = B.Carry;
    c.Tm = B.Tm;
    c.Mc = B.Mc;
    c.U = B.U;
    c.M = B.M;
    c.WK = B.WK;
    c.T = B.T;
    c.U0 = B.U0;
    c.K = B.K;
    c.Ts = B.Ts;
    c.Yd = B.Yd;
    return c;
}

// the pass's largest squaring count: one word, read back on the stream
hipError_t read_smax(const int *smax, int *h_smax, hipStream_t st, int *out) {
    hipError_t e = hipMemcpyAsync(h_smax, smax, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(st);
    *out = *h_smax;
    return e;
}

}  // namespace

hipError_t launch_pipeline(const TiledProblem &TP, const TiledBatch &B, hipStream_t st,
                           const grape_host::KMark &mark) {
    const grape::DevProblem &P = TP.P;
    const Geo g{TP.Pd, P.D};
    const Ctx c = make_ctx(TP, B);
    const size_t img = c.img;
    const int nsteps = B.nb * P.Nt, nchunks = B.nb * TP.Nc, slab = B.X.slab;
    // degree and squaring count of every step; the largest squaring count sizes the launch sequences
    hipError_t e = hipMemsetAsync(B.smax, 0, sizeof(int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tctl, dim3((unsigned)nsteps), dim3(128), 0, st, TP, B.x, (const double *)nullptr, B.ctl,
                       B.smax, (int *)nullptr);
    int smax = 0;
    if ((e = read_smax(B.smax, B.h_smax, st, &smax)) != hipSuccess) return e;
    mark(GRAPE_KERNEL_DEXP, 0);
    for (int s0 = 0; s0 < nsteps; s0 += slab) {
        const int n = std::min(slab, nsteps - s0);
        hipLaunchKernelGGL(k_tgen, dim3((unsigned)n), dim3(NTHREADS), 0, st, TP, B.x, (const double *)nullptr, s0,
                           kNoPert, B.ctl, B.X.A);
        launch_exp_steps(g, B.X, B.ctl + s0, n, B.E + (size_t)s0 * img, smax, st);
    }
    mark(GRAPE_KERNEL_DEXP, 1);
    mark(GRAPE_KERNEL_DSCAN, 0);
    for (int j = 1; j < TP.Lc; ++j) launch_prod<false, false>(g, PipeAddr{c, ST_SCAN, j}, nchunks, st);
    mark(GRAPE_KERNEL_DSCAN, 1);
    mark(GRAPE_KERNEL_DCARRY, 0);
    for (int j = 2; j <= TP.Nc; ++j) launch_prod<false, false>(g, PipeAddr{c, ST_CARRY, j}, B.nb, st);
    const int nhead = B.nb * (1 + P.na);
    hipLaunchKernelGGL(k_ttarget, dim3((unsigned)nhead), dim3(NTHREADS), 0, st, TP, B.x, B.U0);
    launch_prod<true, false>(g, PipeAddr{c, ST_HEADK, 0}, nhead, st);
    hipLaunchKernelGGL(k_thead1, dim3((unsigned)B.nb), dim3(NTHREADS), 0, st, TP, B);
    launch_prod<true, false>(g, PipeAddr{c, ST_HEADT, 0}, B.nb, st);
    const unsigned eb = (unsigned)((img / 2 + NTHREADS - 1) / NTHREADS);
    hipLaunchKernelGGL(k_thead2, dim3(eb, (unsigned)B.nb), dim3(NTHREADS), 0, st, TP, B);
    mark(GRAPE_KERNEL_DCARRY, 1);
    mark(GRAPE_KERNEL_DMC, 0);
    if (TP.Nc > 1) {
        launch_prod<false, false>(g, PipeAddr{c, ST_MC1, 0}, nchunks, st);
        launch_prod<false, true>(g, PipeAddr{c, ST_MC2, 0}, nchunks, st);
    }
    mark(GRAPE_KERNEL_DMC, 1);
    mark(GRAPE_KERNEL_DGRAD, 0);
    for (int s0 = 0; s0 < nsteps; s0 += slab) {
        const int n = std::min(slab, nsteps - s0);
        launch_prod<false, false>(g, PipeAddr{c, ST_Y1, s0}, n, st);
        launch_prod<false, true>(g, PipeAddr{c, ST_Y2, s0}, n, st);
        for (int p = 0; p < P.np; ++p) {
            grape::Pert pp;
            pp.var = grape::VAR_X;
            pp.index = p;
            pp.delta = P.eps;
            hipLaunchKernelGGL(k_tgen, dim3((unsigned)n), dim3(NTHREADS), 0, st, TP, B.x, (const double *)nullptr,
                               s0, pp, B.ctl, B.X.A);
            launch_exp_steps(g, B.X, B.ctl + s0, n, B.Ev, smax, st);
            hipLaunchKernelGGL(k_tcontract, dim3((unsigned)n), dim3(NTHREADS), 0, st, TP, B, s0, p);
        }
    }
    mark(GRAPE_KERNEL_DGRAD, 1);
    return hipGetLastError();
}

hipError_t launch_expm_raw(int d, const double *A, double *E, int n, const ExpSlab &X, int *ctl, int *smax,
                           int *h_smax, int *mstats, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    TiledProblem TP{};
    TP.P.D = d;
    TP.P.Nt = 1;
    TP.Pd = padded_dim(d);
    const Geo g{TP.Pd, d};
    const size_t img = image_doubles(d);
    hipLaunchKernelGGL(k_tctl, dim3((unsigned)n), dim3(128), 0, st, TP, (const double *)nullptr, A, ctl, smax, mstats);
    int sm = 0;
    hipError_t e = read_smax(smax, h_smax, st, &sm);
    if (e != hipSuccess) return e;
    for (int s0 = 0; s0 < n; s0 += X.slab) {
        const int m = std::min(X.slab, n - s0);
        hipLaunchKernelGGL(k_tgen, dim3((unsigned)m), dim3(NTHREADS), 0, st, TP, (const double *)nullptr, A, s0,
                           kNoPert, ctl, X.A);
        launch_exp_steps(g, X, ctl + s0, m, E + (size_t)s0 * img, sm, st);
    }
    return hipGetLastError();
}

}  // namespace grape_tiled
