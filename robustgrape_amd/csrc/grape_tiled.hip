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
// With error sources (GRAPE_OPT_TILED_ERR; launch_err below): the variants of every step through k_tgen and the
// same exponential, k_tstencil, the local-frame images through k_tprod (ErrAddr), then k_twsum, k_tprefix,
// k_terrhead1/2, the conjugations by the carries and the walk B_{k+1} = B_k + W_k M' - M' W_k with k_terrcontract.
// One body each for what the two paths share: launch_variant_exp (k_tgen, then the exponential's launches) and
// target_rows (the x_add rows of k_thead1 and k_terrhead1).
#include "grape_tiled.hpp"
#include "grape_tiled_api.hpp"

namespace grape_tiled {

namespace {

constexpr grape::Pert kNoPert = {-1, 0, 0.0};
constexpr grape::VSpec kNominal = {{-1, 0, 0.0}, -1, 0.0};

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
// -i dt c_t of every term of variant vs of step k into LDS: H0's terms, then errval x the terms of source vs.err
// (UnitaryCalculations.jl:45-97: the perturbed variable in both).  Returns the term count (at most kMaxTerms:
// validate_desc, choose_route).
__device__ __forceinline__ int stage_coefs(const grape::DevProblem &P, const double *xb, int k,
                                           const grape::VSpec &vs, double *gre, double *gim, int *gop) {
    const double *xk = xb + (size_t)k * P.np;
    const double *xadd = xb + (size_t)P.np * P.Nt;
    auto put = [&](int t, int op, cd c) {  // -i dt c into slot t
        gre[t] = P.dt * c.im;
        gim[t] = -(P.dt * c.re);
        gop[t] = op;
    };
    for (int t = threadIdx.x; t < P.n_h0; t += blockDim.x) {
        const Term tm = P.h0[t];
        put(t, tm.op, grape::term_coef(tm, k + 1, xk, xadd, vs.pert));
    }
    int n = P.n_h0;
    if (vs.err >= 0) {
        const int t0 = P.err_off[vs.err], ne = P.err_off[vs.err + 1] - t0;
        for (int t = threadIdx.x; t < ne; t += blockDim.x) {
            const Term tm = P.err[t0 + t];
            put(n + t, tm.op, grape::cscale(vs.errval, grape::term_coef(tm, k + 1, xk, xadd, vs.pert)));
        }
        n += ne;
    }
    __syncthreads();
    return n;
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
    if (!raw) stage_coefs(P, x + (size_t)(item / P.Nt) * P.nx, item % P.Nt, kNominal, gre, gim, gop);
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

// A / 2^s of every item of a slab (item i = step s0 + i of the pass, variant vs: one control perturbed and / or
// an error source added; or the raw image s0 + i), s from the step's ctl word: every eps, eps2, error and mixed
// variant is scaled -- and later expanded and squared -- exactly as its nominal, so that no stencil sees the
// difference of two roundings.
__global__ __launch_bounds__(NTHREADS) void k_tgen(TiledProblem TP, const double *x, const double *raw, int s0,
                                                    grape::VSpec vs, const int *ctl, double *A) {
    __shared__ double gre[kMaxTerms], gim[kMaxTerms];
    __shared__ int gop[kMaxTerms];
    const grape::DevProblem &P = TP.P;
    const int i = blockIdx.x, step = s0 + i, Pd = TP.Pd;
    const size_t plane = (size_t)Pd * Pd, img = 2 * plane;
    int nterms = 0;
    if (!raw) nterms = stage_coefs(P, x + (size_t)(step / P.Nt) * P.nx, step % P.Nt, vs, gre, gim, gop);
    const double sc = ldexp(1.0, -(ctl[step] >> 2));
    double *dst = A + (size_t)i * img;
    for (size_t a = threadIdx.x; a < plane; a += NTHREADS) {
        double re, im;
        if (raw) {
            re = raw[(size_t)step * img + a];
            im = raw[(size_t)step * img + plane + a];
        } else {
            sum_terms(TP.opimg, img, plane, a, nterms, gre, gim, gop, re, im);
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

// variant vs of the n steps from s0 of the pass (raw: the images s0 ...): A / 2^s, then its exponential into out
void launch_variant_exp(const TiledProblem &TP, const Geo &g, const double *x, const double *raw, int s0, int n,
                        const grape::VSpec &vs, const int *ctl, const ExpSlab &X, double *out, int smax,
                        hipStream_t st) {
    hipLaunchKernelGGL(k_tgen, dim3((unsigned)n), dim3(NTHREADS), 0, st, TP, x, raw, s0, vs, ctl, X.A);
    launch_exp_steps(g, X, ctl + s0, n, out, smax, st);
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

// The target rows of a head: out[q] = (scale (2 sum_ij W_i P_j Re(conj(K_ij) Kd_ij) + 2 Re(conj(tau) tr(W Kd)))) / DD
// for the na images Kd_q that follow K = Kv[0].  K = U0^dag U, scale 1: F_dx_add's target part
// (FidelityCalculations.jl:67-76); K = Ke, tau = tau_e, scale 2: F_d2err_dx_add's (:96-113)
__device__ __forceinline__ void target_rows(const TiledProblem &TP, const double *Kv, double tau_re, double tau_im,
                                            double scale, double *out, double *red) {
    const grape::DevProblem &P = TP.P;
    const int Pd = TP.Pd;
    const size_t plane = (size_t)Pd * Pd, img = 2 * plane;
    for (int q = 0; q < P.na; ++q) {
        const double *Kd = Kv + (size_t)(1 + q) * img;
        double pr = 0.0, dre = 0.0, dim = 0.0;
        for (size_t a = threadIdx.x; a < plane; a += NTHREADS) {
            const int row = (int)(a / Pd), col = (int)(a % Pd);
            const double wr = TP.W[row], pcol = TP.W[col] != 0.0 ? 1.0 : 0.0;
            pr += wr * (pcol * (Kd[a] * Kv[a] + Kd[plane + a] * Kv[plane + a]));
            if (row == col) {
                dre += wr * Kd[a];
                dim += wr * Kd[plane + a];
            }
        }
        const double s1 = wg_sum(pr, red), tr_re = wg_sum(dre, red), tr_im = wg_sum(dim, red);
        if (threadIdx.x == 0) out[q] = (scale * (2.0 * s1 + 2.0 * (tau_re * tr_re + tau_im * tr_im))) / P.DD;
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
    target_rows(TP, K, tau_re, tau_im, 1.0, B.Fdx + (size_t)b * P.nx + (size_t)P.np * P.Nt, red);
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

// ---------------------------------------------------------------------------
// error sources (GRAPE_OPT_TILED_ERR): F_d2err and F_d2err_dx.  Algebra: grape_errpath.hpp header; stage
// order: grape_dense.hip (k_dlocal, k_dwsum, k_derr_scan, k_dmce, k_derr_grad).  The local-frame images are
// stored conjugate-transposed, Zd = Z^dag = Q_{k-1}^dag dX^dag Q_k: Re tr(A Z) = sum Re(A) o Re(Zd) + Im(A) o
// Im(Zd) is elementwise, and W_k enters the walk's products through op().  F_dx comes from Z1 too
// (Re tr(M'_c Z1), the dense engine's form), not from the nerr == 0 pipeline's Y_k.
// ---------------------------------------------------------------------------
struct ErrCtx {
    Ctx c;
    int np, ne, nz;
    double *Zl, *dX, *Sd, *Tmp, *Vc, *Sx, *Dx, *Mce, *Tce, *Dce, *Bst, *Lam, *Tot, *Ue, *UeU, *KW, *Me, *Ke;
    __device__ double *zimg(int b, int k, int slot) const {
        return Zl + (((size_t)b * c.Nt + k) * nz + slot) * c.img;
    }
    // item i = (b ne + e) Nc + chunk of the per-chunk stages; chunk 0 (Carry = I) aliases the global-frame images
    __device__ double *mce(int i) const {
        return (i % c.Nc) == 0 ? Me + (size_t)(i / c.Nc) * c.img : Mce + (size_t)i * c.img;
    }
    __device__ double *tce(int i) const { return ((i % c.Nc) == 0 ? Sx : Tce) + (size_t)i * c.img; }
    __device__ double *dce(int i) const { return ((i % c.Nc) == 0 ? Dx : Dce) + (size_t)i * c.img; }
};

enum ErrStage { ES_L1, ES_L2, ES_V1, ES_V2, ES_UE, ES_KE, ES_UEU, ES_KW, ES_C1, ES_C2, ES_B1, ES_B2, ES_W1, ES_W2 };

// the epilogue of grape_tiled.hpp as C = c1 X + op(L) op(R)
__device__ __forceinline__ void add_image(Ops &o, const double *X, double c1) {
    o.X1 = o.X2 = o.X3 = X;
    o.c1 = c1;
}

// The error path's product stages: a functor of its own, so that the kernels of the nerr == 0 pipeline keep
// their code.
struct ErrAddr {
    ErrCtx c;
    int stage;
    int j;     // ES_L1 / ES_L2: first step of the slab; ES_C1 / ES_C2: which image; ES_W1 / ES_W2: position in the chunk
    int slot;  // ES_L1 / ES_L2: the local-frame slot written
    __device__ bool operator()(int i, Ops &o) const {
        const Ctx &p = c.c;
        const size_t img = p.img;
        switch (stage) {
        case ES_L1:
        case ES_L2: {  // item = step j + i of the pass: T = dX^dag Q_k, Zd = Q_{k-1}^dag T (chunk start: Zd = T)
            const int step = j + i, b = step / p.Nt, k = step % p.Nt;
            const bool first = (k % p.Lc) == 0;
            double *ts = p.Ts + (size_t)i * img;
            if (stage == ES_L1) {
                o.L = c.dX + (size_t)i * img;
                o.R = p.qimg(b, k);
                o.C = first ? c.zimg(b, k, slot) : ts;
            } else {
                if (first) return false;
                o.L = p.qimg(b, k - 1);
                o.R = ts;
                o.C = c.zimg(b, k, slot);
            }
            return true;
        }
        case ES_V1:
        case ES_V2: {  // item (b, e, chunk >= 1): (sum W) Carry = Sd^dag Carry, then Vc = Carry^dag (.)
            const int ch = i % p.Nc, b = i / (p.Nc * c.ne);
            if (ch == 0) return false;  // (k_twsum wrote Vc_0 = sum W)
            if (stage == ES_V1) {
                o.L = c.Sd + (size_t)i * img;
                o.R = p.carry(b, ch);
                o.C = c.Tmp + (size_t)i * img;
            } else {
                o.L = p.carry(b, ch);
                o.R = c.Tmp + (size_t)i * img;
                o.C = c.Vc + (size_t)i * img;
            }
            return true;
        }
        case ES_UE: {  // item (b, e): U_derr = U Tot                                  UnitaryCalculations.jl:122-123
            o.L = p.uimg(i / c.ne);
            o.R = c.Tot + (size_t)i * img;
            o.C = c.Ue + (size_t)i * img;
            return true;
        }
        case ES_KE: {  // item (b, e, v): Ke = U0^dag Ue, Kde_q = dU0_q^dag Ue
            const int nh = 1 + p.na, v = i % nh, be = i / nh, b = be / c.ne;
            o.L = p.U0 + ((size_t)b * nh + v) * img;
            o.R = c.Ue + (size_t)be * img;
            o.C = c.Ke + (size_t)i * img;
            return true;
        }
        case ES_UEU: {  // item (b, e): Ue^dag U
            o.L = c.Ue + (size_t)i * img;
            o.R = p.uimg(i / c.ne);
            o.C = c.UeU + (size_t)i * img;
            return true;
        }
        case ES_KW: {  // item (b, e): Ke^dag (W K)
            o.L = c.Ke + (size_t)i * (1 + p.na) * img;
            o.R = p.WK + (size_t)(i / c.ne) * img;
            o.C = c.KW + (size_t)i * img;
            return true;
        }
        case ES_C1:
        case ES_C2: {  // item (b, e, chunk >= 1): Carry X, then (Carry X) Carry^dag; X = M_e, S_c, Tot - S_c (j = 0, 1, 2)
            const int ch = i % p.Nc, be = i / p.Nc, b = be / c.ne;
            if (ch == 0) return false;
            double *tm = c.Tmp + (size_t)i * img;
            if (stage == ES_C1) {
                o.L = p.carry(b, ch);
                o.R = j == 0 ? c.Me + (size_t)be * img : (j == 1 ? c.Sx : c.Dx) + (size_t)i * img;
                o.C = tm;
            } else {
                o.L = tm;
                o.R = p.carry(b, ch);
                o.C = (j == 0 ? c.Mce : j == 1 ? c.Tce : c.Dce) + (size_t)i * img;
            }
            return true;
        }
        case ES_B1: {  // item (b, e, chunk): T_c M'
            o.L = c.tce(i);
            o.R = c.mce(i);
            o.C = c.Lam + (size_t)i * img;
            return true;
        }
        case ES_B2: {  // B at the chunk start: [T_c, M'] + M' Ttot = T_c M' + M' (Ttot - T_c)
            o.L = c.mce(i);
            o.R = c.dce(i);
            o.C = c.Bst + (size_t)i * img;
            add_image(o, c.Lam + (size_t)i * img, 1.0);
            return true;
        }
        default: {  // ES_W1 / ES_W2, item (b, e, chunk), step k = chunk Lc + j: the walk keeps -Lambda_k, so that both
                    // products add:  -Lambda_k = -B_k + M' W_k,  B_{k+1} = -(-Lambda_k) + W_k M'
            const int ch = i % p.Nc, be = i / p.Nc, b = be / c.ne, e = be % c.ne, k = ch * p.Lc + j;
            if (k >= p.Nt) return false;
            double *wd = c.zimg(b, k, c.np + e);  // W_k^dag
            if (stage == ES_W1) {
                o.L = c.mce(i);
                o.R = wd;
                o.C = c.Lam + (size_t)i * img;
                add_image(o, c.Bst + (size_t)i * img, -1.0);
            } else {
                o.L = wd;
                o.R = c.mce(i);
                o.C = c.Bst + (size_t)i * img;
                add_image(o, c.Lam + (size_t)i * img, -1.0);
            }
            return true;
        }
        }
    }
};

// the stencils of a slab, elementwise and left to right as the reference writes them (item i = step s0 + i):
//   u < 0:  dX = (E' - E) / eps                                    UnitaryCalculations.jl:48-75
//   u >= 0: dX = ((E_mix + E) - E_err2 - E_dx2_u) / eps2^2          UnitaryCalculations.jl:79-95
__global__ __launch_bounds__(NTHREADS) void k_tstencil(TiledProblem TP, TiledBatch B, int s0, int u) {
    const grape::DevProblem &P = TP.P;
    const int i = blockIdx.x;
    const size_t img = 2 * (size_t)TP.Pd * TP.Pd, slab = (size_t)B.X.slab;
    const double *E = B.E + (size_t)(s0 + i) * img, *Ev = B.Ev + (size_t)i * img;
    double *dX = B.Yd + (size_t)i * img;
    if (u < 0) {
        for (size_t a = threadIdx.x; a < img; a += NTHREADS) dX[a] = (Ev[a] - E[a]) * P.inv_eps;
    } else {
        const double *e2 = B.Eh + ((size_t)P.np * slab + i) * img, *d2 = B.Eh + ((size_t)u * slab + i) * img;
        for (size_t a = threadIdx.x; a < img; a += NTHREADS)
            dX[a] = (((Ev[a] + E[a]) - e2[a]) - d2[a]) * P.inv_eps2sq;
    }
}

// F_dx[u, k] = Re tr(M'_c Z1_{k,u}); item i = step s0 + i of the pass              FidelityCalculations.jl:56-65
__global__ __launch_bounds__(NTHREADS) void k_tzcontract(TiledProblem TP, TiledBatch B, int s0, int u) {
    __shared__ double red[NTHREADS];
    const grape::DevProblem &P = TP.P;
    const int step = s0 + blockIdx.x, b = step / P.Nt, k = step % P.Nt, ch = k / TP.Lc;
    const size_t img = 2 * (size_t)TP.Pd * TP.Pd;
    const double *Mc = ch == 0 ? B.M + (size_t)b * img : B.Mc + ((size_t)b * TP.Nc + ch) * img;
    const double *Zd = B.Zl + ((size_t)step * P.nz + u) * img;
    double acc = 0.0;
    for (size_t a = threadIdx.x; a < img; a += NTHREADS) acc += Mc[a] * Zd[a];
    const double s = wg_sum(acc, red);
    if (threadIdx.x == 0) B.Fdx[(size_t)b * P.nx + (size_t)k * P.np + u] = s;
}

// item (b, e, chunk): the chunk's sum of W_k^dag in step order; chunk 0 (Carry = I) writes Vc_0 = sum W itself,
// the others (sum W)^dag for ES_V1
__global__ __launch_bounds__(NTHREADS) void k_twsum(TiledProblem TP, TiledBatch B) {
    const grape::DevProblem &P = TP.P;
    const int i = blockIdx.x, ch = i % TP.Nc, be = i / TP.Nc, e = be % P.ne, b = be / P.ne, Pd = TP.Pd;
    const size_t plane = (size_t)Pd * Pd, img = 2 * plane;
    const int k0 = ch * TP.Lc, k1 = min(k0 + TP.Lc, P.Nt);
    const double *Wd = B.Zl + (((size_t)b * P.Nt + k0) * P.nz + P.np + e) * img;
    const size_t stride = (size_t)P.nz * img;
    for (size_t a = threadIdx.x; a < plane; a += NTHREADS) {
        double re = 0.0, im = 0.0;
        for (int k = k0; k < k1; ++k) {
            re += Wd[(size_t)(k - k0) * stride + a];
            im += Wd[(size_t)(k - k0) * stride + plane + a];
        }
        if (ch == 0) {
            const size_t at = (a % Pd) * Pd + a / Pd;
            B.Vc[(size_t)i * img + at] = re;
            B.Vc[(size_t)i * img + plane + at] = -im;
        } else {
            B.Sd[(size_t)i * img + a] = re;
            B.Sd[(size_t)i * img + plane + a] = im;
        }
    }
}

// item (b, e): the exclusive prefix S_c of Vc over the chunks, Tot, and Tot - S_c         UnitaryCalculations.jl:111-113
__global__ __launch_bounds__(NTHREADS) void k_tprefix(TiledProblem TP, TiledBatch B) {
    const int be = blockIdx.y, Nc = TP.Nc;
    const size_t img = 2 * (size_t)TP.Pd * TP.Pd, a = (size_t)blockIdx.x * NTHREADS + threadIdx.x;
    if (a >= img) return;
    const size_t base = (size_t)be * Nc * img + a;
    double run = 0.0;
    for (int c = 0; c < Nc; ++c) {
        B.Sx[base + (size_t)c * img] = run;
        run += B.Vc[base + (size_t)c * img];
    }
    B.Tot[(size_t)be * img + a] = run;
    for (int c = 0; c < Nc; ++c) B.Dx[base + (size_t)c * img] = run - B.Sx[base + (size_t)c * img];
}

// per (b, e): tau_e = tr(W Ke), F_d2err, and the target rows of F_d2err_dx             FidelityCalculations.jl:78-83, 96-113
__global__ __launch_bounds__(NTHREADS) void k_terrhead1(TiledProblem TP, TiledBatch B) {
    __shared__ double red[NTHREADS];
    const grape::DevProblem &P = TP.P;
    const int be = blockIdx.x, Pd = TP.Pd, nh = 1 + P.na;
    const size_t plane = (size_t)Pd * Pd, img = 2 * plane;
    const double *Ke = B.Ke + (size_t)be * nh * img, *Ue = B.Ue + (size_t)be * img;
    double a1 = 0.0, a2 = 0.0, tre = 0.0, tim = 0.0;
    for (size_t a = threadIdx.x; a < plane; a += NTHREADS) {
        const int row = (int)(a / Pd), col = (int)(a % Pd);
        const double wr = TP.W[row], wc = TP.W[col], pcol = wc != 0.0 ? 1.0 : 0.0;
        const double kr = Ke[a], ki = Ke[plane + a], ur = Ue[a], ui = Ue[plane + a];
        a1 += wr * (pcol * (kr * kr + ki * ki));
        a2 += wc * (ur * ur + ui * ui);  // W_j (Ue^dag Ue)_jj
        if (row == col) {
            tre += wr * kr;
            tim += wr * ki;
        }
    }
    const double s_a1 = wg_sum(a1, red), s_a2 = wg_sum(a2, red);
    const double te_re = wg_sum(tre, red), te_im = wg_sum(tim, red);
    if (threadIdx.x == 0) {
        // F_d2err = 2[sum W_i P_j |Ke_ij|^2 - (1+D) sum W (Ue^dag Ue)_ii + |te|^2] / (D(D+1))
        B.Fd2[be] = 2.0 * (s_a1 - (1.0 + P.Dtr) * s_a2 + te_re * te_re + te_im * te_im) / P.DD;
        B.taue[2 * be] = te_re;
        B.taue[2 * be + 1] = te_im;
    }
    target_rows(TP, Ke, te_re, te_im, 2.0, B.Fd2dx + (size_t)be * P.nx + (size_t)P.np * P.Nt, red);
}

// M_e = (4 / DD) [P Ke^dag W K + conj(tau_e) W K - (1 + D) W Ue^dag U]
__global__ __launch_bounds__(NTHREADS) void k_terrhead2(TiledProblem TP, TiledBatch B) {
    const grape::DevProblem &P = TP.P;
    const int be = blockIdx.y, b = be / P.ne, Pd = TP.Pd;
    const size_t plane = (size_t)Pd * Pd, img = 2 * plane;
    const size_t a = (size_t)blockIdx.x * NTHREADS + threadIdx.x;
    if (a >= plane) return;
    const double te_re = B.taue[2 * be], te_im = B.taue[2 * be + 1], sc = 4.0 / P.DD;
    const double wr = TP.W[a / Pd], prow = wr != 0.0 ? 1.0 : 0.0;
    const double *KW = B.KW + (size_t)be * img, *WK = B.WK + (size_t)b * img, *UeU = B.UeU + (size_t)be * img;
    const double wkr = WK[a], wki = WK[plane + a];
    const double cr = te_re * wkr + te_im * wki, ci = te_re * wki - te_im * wkr;  // conj(tau_e) W K
    const double ur = (1.0 + P.Dtr) * wr * UeU[a], ui = (1.0 + P.Dtr) * wr * UeU[plane + a];
    double *Me = B.Me + (size_t)be * img;
    Me[a] = sc * (prow * KW[a] + cr - ur);
    Me[plane + a] = sc * (prow * KW[plane + a] + ci - ui);
}

// F_d2err_dx[u, k, e] = Re[tr(Lambda_k Z1_{k,u}) + tr(M' Z2_{k,e,u})], k = chunk Lc + j; item ((b, e, chunk), u);
// B.Lam holds -Lambda_k (ES_W1)
__global__ __launch_bounds__(NTHREADS) void k_terrcontract(TiledProblem TP, TiledBatch B, int j) {
    __shared__ double red[NTHREADS];
    const grape::DevProblem &P = TP.P;
    const int u = blockIdx.x % P.np, i = blockIdx.x / P.np, ch = i % TP.Nc, be = i / TP.Nc, e = be % P.ne, b = be / P.ne;
    const int k = ch * TP.Lc + j;
    if (k >= P.Nt) return;
    const size_t img = 2 * (size_t)TP.Pd * TP.Pd;
    const double *Zk = B.Zl + ((size_t)b * P.Nt + k) * P.nz * img;
    const double *Z1 = Zk + (size_t)u * img, *Z2 = Zk + (size_t)(P.np + P.ne + e * P.np + u) * img;
    const double *nLam = B.Lam + (size_t)i * img;
    const double *Mp = ch == 0 ? B.Me + (size_t)be * img : B.Mce + (size_t)i * img;
    double acc = 0.0;
    for (size_t a = threadIdx.x; a < img; a += NTHREADS) acc += Mp[a] * Z2[a] - nLam[a] * Z1[a];
    const double s = wg_sum(acc, red);
    if (threadIdx.x == 0) B.Fd2dx[(size_t)be * P.nx + (size_t)k * P.np + u] = s;
}

ErrCtx make_err_ctx(const TiledProblem &TP, const TiledBatch &B, const Ctx &c) {
    ErrCtx e;
    e.c = c;
    e.np = TP.P.np;
    e.ne = TP.P.ne;
    e.nz = TP.P.nz;
    e.Zl = B.Zl;
    e.dX = B.Yd;  // (the nerr == 0 pipeline's Y^dag buffer holds the slab's stencil)
    e.Sd = B.Sd;
    e.Tmp = B.Tmp;
    e.Vc = B.Vc;
    e.Sx = B.Sx;
    e.Dx = B.Dx;
    e.Mce = B.Mce;
    e.Tce = B.Tce;
    e.Dce = B.Dce;
    e.Bst = B.Bst;
    e.Lam = B.Lam;
    e.Tot = B.Tot;
    e.Ue = B.Ue;
    e.UeU = B.UeU;
    e.KW = B.KW;
    e.Me = B.Me;
    e.Ke = B.Ke;
    return e;
}

// After the nominal pipeline's head (M'_c of every chunk): the variants of every slab into the local-frame
// images, the sums and the error head, the error gradient's walk.  Per step 2 np + ne (2 + np) exponentials and
// 2 (np + ne + ne np) products; per chunk and source 2 Lc walk products and 12 of the conjugations.
hipError_t launch_err(const TiledProblem &TP, const TiledBatch &B, const Geo &g, const Ctx &c, int smax, hipStream_t st,
                      const grape_host::KMark &mark) {
    const grape::DevProblem &P = TP.P;
    const ErrCtx ec = make_err_ctx(TP, B, c);
    const size_t img = c.img;
    const int np = P.np, ne = P.ne, nsteps = B.nb * P.Nt, slab = B.X.slab;
    const int nbe = B.nb * ne, nbec = nbe * TP.Nc;
    mark(GRAPE_KERNEL_GRAD, 0);
    for (int s0 = 0; s0 < nsteps; s0 += slab) {
        const int n = std::min(slab, nsteps - s0);
        auto variant = [&](int var, int index, double delta, int err, double errval, double *out) {
            launch_variant_exp(TP, g, B.x, nullptr, s0, n, {{var, index, delta}, err, errval}, B.ctl, B.X, out, smax, st);
        };
        auto local = [&](int u, int slot) {  // the stencil of B.Ev into slot
            hipLaunchKernelGGL(k_tstencil, dim3((unsigned)n), dim3(NTHREADS), 0, st, TP, B, s0, u);
            launch_prod<true, false>(g, ErrAddr{ec, ES_L1, s0, slot}, n, st);
            launch_prod<true, false>(g, ErrAddr{ec, ES_L2, s0, slot}, n, st);
        };
        for (int u = 0; u < np; ++u) variant(grape::VAR_X, u, P.eps2, -1, 0.0, B.Eh + (size_t)u * slab * img);
        for (int u = 0; u < np; ++u) {
            variant(grape::VAR_X, u, P.eps, -1, 0.0, B.Ev);
            local(-1, u);  // Z1_u
            hipLaunchKernelGGL(k_tzcontract, dim3((unsigned)n), dim3(NTHREADS), 0, st, TP, B, s0, u);
        }
        for (int e = 0; e < ne; ++e) {
            variant(-1, 0, 0.0, e, P.eps, B.Ev);
            local(-1, np + e);  // W_e
            variant(-1, 0, 0.0, e, P.eps2, B.Eh + (size_t)np * slab * img);
            for (int u = 0; u < np; ++u) {
                variant(grape::VAR_X, u, P.eps2, e, P.eps2, B.Ev);
                local(u, np + ne + e * np + u);  // Z2_{e,u}
            }
        }
    }
    mark(GRAPE_KERNEL_GRAD, 1);
    mark(GRAPE_KERNEL_ERR_SCAN, 0);
    hipLaunchKernelGGL(k_twsum, dim3((unsigned)nbec), dim3(NTHREADS), 0, st, TP, B);
    if (TP.Nc > 1) {
        launch_prod<true, false>(g, ErrAddr{ec, ES_V1, 0, 0}, nbec, st);
        launch_prod<true, false>(g, ErrAddr{ec, ES_V2, 0, 0}, nbec, st);
    }
    const unsigned eb = (unsigned)((img / 2 + NTHREADS - 1) / NTHREADS);
    hipLaunchKernelGGL(k_tprefix, dim3(2 * eb, (unsigned)nbe), dim3(NTHREADS), 0, st, TP, B);
    launch_prod<false, false>(g, ErrAddr{ec, ES_UE, 0, 0}, nbe, st);
    launch_prod<true, false>(g, ErrAddr{ec, ES_KE, 0, 0}, nbe * (1 + P.na), st);
    launch_prod<true, false>(g, ErrAddr{ec, ES_UEU, 0, 0}, nbe, st);
    hipLaunchKernelGGL(k_terrhead1, dim3((unsigned)nbe), dim3(NTHREADS), 0, st, TP, B);
    launch_prod<true, false>(g, ErrAddr{ec, ES_KW, 0, 0}, nbe, st);
    hipLaunchKernelGGL(k_terrhead2, dim3(eb, (unsigned)nbe), dim3(NTHREADS), 0, st, TP, B);
    if (TP.Nc > 1)
        for (int which = 0; which < 3; ++which) {
            launch_prod<false, false>(g, ErrAddr{ec, ES_C1, which, 0}, nbec, st);
            launch_prod<false, true>(g, ErrAddr{ec, ES_C2, which, 0}, nbec, st);
        }
    launch_prod<false, false>(g, ErrAddr{ec, ES_B1, 0, 0}, nbec, st);
    launch_prod<false, false>(g, ErrAddr{ec, ES_B2, 0, 0}, nbec, st);
    mark(GRAPE_KERNEL_ERR_SCAN, 1);
    mark(GRAPE_KERNEL_ERR_GRAD, 0);
    for (int j = 0; j < TP.Lc; ++j) {
        launch_prod<false, true>(g, ErrAddr{ec, ES_W1, j, 0}, nbec, st);
        hipLaunchKernelGGL(k_terrcontract, dim3((unsigned)(nbec * np)), dim3(NTHREADS), 0, st, TP, B, j);
        if (j + 1 < TP.Lc) launch_prod<true, false>(g, ErrAddr{ec, ES_W2, j, 0}, nbec, st);
    }
    mark(GRAPE_KERNEL_ERR_GRAD, 1);
    return hipGetLastError();
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
        launch_variant_exp(TP, g, B.x, nullptr, s0, n, kNominal, B.ctl, B.X, B.E + (size_t)s0 * img, smax, st);
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
    if (P.ne > 0) return launch_err(TP, B, g, c, smax, st, mark);  // (F_dx from Z1 there)
    mark(GRAPE_KERNEL_DGRAD, 0);
    for (int s0 = 0; s0 < nsteps; s0 += slab) {
        const int n = std::min(slab, nsteps - s0);
        launch_prod<false, false>(g, PipeAddr{c, ST_Y1, s0}, n, st);
        launch_prod<false, true>(g, PipeAddr{c, ST_Y2, s0}, n, st);
        for (int p = 0; p < P.np; ++p) {
            launch_variant_exp(TP, g, B.x, nullptr, s0, n, {{grape::VAR_X, p, P.eps}, -1, 0.0}, B.ctl, B.X, B.Ev, smax, st);
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
        launch_variant_exp(TP, g, nullptr, A, s0, m, kNominal, ctl, X, E + (size_t)s0 * img, sm, st);
    }
    return hipGetLastError();
}

}  // namespace grape_tiled
