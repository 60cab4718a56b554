// grape_plan_build.hip -- plan construction: the dense and tiled plans, and the phases of a small-engine /
// general-path plan (grape_plan_create, grape_engine.hip, calls them).  Allocation, uploads and the
// once-per-plan table fills; the decisions they act on come from grape_descriptor.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "grape_plan.hpp"

namespace grape_eng {

// Chunk count of the 3-level phase-covariant class on throughput passes (the merged walks' chunking,
// grape_walk.hpp k_walk_fwd_m / k_walk_grad_m).  A walk's time is (rounds of resident waves) x (steps
// per lane): every lane of a pass walks L steps, so a chunk count that leaves the last round of waves
// partly empty wastes that round's SIMD time -- C2's 10 chunks at 32 768 evaluations per pass were
// 5 120 gradient waves, 2.5 rounds at 2 waves per SIMD.  The model, in microseconds per C2 unit from
// the round-5 profile (profiles/r05/final_c2b): 2.72 x rounds(grad, 2 waves/SIMD) x L + 5.7 x chunks
// (k_scan_seq), minimised over [nc/2, 2 nc]; the forward walk measured the same at 8, 10, 12 and 16
// chunks (0.185-0.187 ms per pass), so it has no term.  C2: 8 chunks, 48.5-48.9 -> 50.7 M evals/s
// (12: 49.7 M, 16: 48.9 M; profiles/r05/ab_nchunks).  GRAPE_GAUGE_NCHUNKS=n (environment) forces n.
static int merged_chunk_count(long MB, int Nt, int nc, int ncu) {
    if (const char *e = getenv("GRAPE_GAUGE_NCHUNKS")) {
        const int n = atoi(e);
        if (n > 0) return std::min(n, Nt);
    }
    const double simds = 4.0 * ncu;
    double best = 1e300;
    int pick = nc;
    for (int n = std::max(1, nc / 2); n <= std::min(2 * nc, Nt); ++n) {
        const int L = (Nt + n - 1) / n, nch = (Nt + L - 1) / L;
        const double waves = std::ceil((double)MB * nch / 64.0);
        const double cost = 2.72 * std::ceil(waves / (2.0 * simds)) * L + 5.7 * nch;
        if (cost < best - 1e-9) {
            best = cost;
            pick = nch;
        }
    }
    return pick;
}

// ---------------------------------------------------------------------------
// dense engine plan (GRAPE_MAX_SMALL_DIM < d <= GRAPE_MAX_DENSE_DIM)
// ---------------------------------------------------------------------------
// column-major interleaved d x d complex <-> zero-padded 64 x 64 register-file image:
// f(o, e) for every image slot o (re at o, im at 64 * 64 + o) and its element's offset e (-1: padding)
template <class F>
static void dense_image_slots(int d, F &&f) {
    for (int w = 0; w < 4; ++w)
        for (int t = 0; t < 4; ++t)
            for (int r = 0; r < 4; ++r)
                for (int l = 0; l < 64; ++l) {
                    const int row = 16 * t + (l >> 4) + 4 * r, col = 16 * w + (l & 15);
                    f(((w * 4 + t) * 4 + r) * 64 + l, row < d && col < d ? 2 * ((long)row + (long)col * d) : -1L);
                }
}
void to_dense_image(const double *src, int d, double *img) {
    dense_image_slots(d, [&](int o, long e) {
        img[o] = e >= 0 ? src[e] : 0.0;
        img[64 * 64 + o] = e >= 0 ? src[e + 1] : 0.0;
    });
}
void from_dense_image(const double *img, int d, double *dst) {
    dense_image_slots(d, [&](int o, long e) {
        if (e >= 0) dst[e] = img[o], dst[e + 1] = img[64 * 64 + o];
    });
}

// uploads the general-projector matrices and sets P.gen_proj / PA / PB / P0g
static int upload_projector(grape_plan *p, const ProjectorSetup &ps, DevProblem &P, size_t scratch_blocks) {
    P.gen_proj = ps.general ? 1 : 0;
    if (!ps.general) return GRAPE_OK;
    const size_t T = ps.A.size();
    if (p->mem.alloc(&p->d_PA, T) != hipSuccess || p->mem.alloc(&p->d_PB, T) != hipSuccess || p->mem.alloc(&p->d_P0g, T) != hipSuccess ||
        p->mem.alloc(&p->d_gpscr, scratch_blocks * grape_proj::kScratchSlots * T) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (general projector)");
    if (hipMemcpy(p->d_PA, ps.A.data(), T * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->d_PB, ps.B.data(), T * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->d_P0g, ps.P0.data(), T * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "upload failed (general projector)");
    P.PA = p->d_PA;
    P.PB = p->d_PB;
    P.P0g = p->d_P0g;
    return GRAPE_OK;
}

// the scalars of a plan's problem that come straight from the descriptor (every engine)
static void fill_problem_scalars(const grape_desc *desc, double trP, DevProblem &P) {
    P.D = desc->ndim;
    P.opts = desc->reserved[1];
    P.Nt = desc->ntimes;
    P.np = desc->nparam;
    P.na = desc->nadd;
    P.ne = desc->nerr;
    P.nx = desc->nparam * desc->ntimes + desc->nadd;
    P.n_h0 = desc->n_h0_terms;
    P.n_tgt = desc->n_target_terms;
    P.dt = desc->t0 / desc->ntimes;
    P.eps = desc->eps;
    P.eps2 = desc->eps2;
    P.inv_eps = 1.0 / desc->eps;
    P.inv_eps2sq = 1.0 / (desc->eps2 * desc->eps2);
    P.DD = trP * (trP + 1.0);
    P.Dtr = trP;
}

// the variant list of P's scalars (grape_plan_setup.hpp build_variants) and its layout into P
static std::vector<grape::VSpec> set_variants(DevProblem &P, int nxa, bool with_grad_variants) {
    grape_setup::Variants V = grape_setup::build_variants(P.np, nxa, P.ne, P.eps, P.eps2, with_grad_variants);
    P.off_dx = V.off_dx;
    P.off_dxa = V.off_dxa;
    P.off_dx2 = V.off_dx2;
    P.off_err = V.off_err;
    P.err_stride = V.err_stride;
    return std::move(V.vs);
}

// Device copies of the term lists, the error offsets and the variant list, and their pointers in P
// (d_err / d_err_off: plans with error sources; host-table plans upload no terms).  sfx / err_sfx name
// the engine in the messages.
static int upload_terms(grape_plan *p, const grape_desc *desc, int n_err_terms, const std::vector<grape::VSpec> &vs,
                        DevProblem &P, const char *sfx, const char *err_sfx) {
    const int ne = desc->nerr;
    bool ok = p->mem.alloc(&p->d_h0, std::max(desc->n_h0_terms, 0)) == hipSuccess &&
              p->mem.alloc(&p->d_tgt, std::max(desc->n_target_terms, 0)) == hipSuccess &&
              p->mem.alloc(&p->d_vs, vs.size()) == hipSuccess;
    if (ok && ne > 0)
        ok = p->mem.alloc(&p->d_err, (size_t)n_err_terms) == hipSuccess &&
             p->mem.alloc(&p->d_err_off, (size_t)ne + 1) == hipSuccess;
    if (!ok) return fail(GRAPE_ERR_ALLOC, std::string("device allocation failed") + sfx);
    if (hipMemcpy(p->d_vs, vs.data(), vs.size() * sizeof(grape::VSpec), hipMemcpyHostToDevice) != hipSuccess ||
        (!p->tables &&
         (hipMemcpy(p->d_h0, desc->h0_terms, desc->n_h0_terms * sizeof(Term), hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(p->d_tgt, desc->target_terms, desc->n_target_terms * sizeof(Term), hipMemcpyHostToDevice) !=
              hipSuccess)))
        return fail(GRAPE_ERR_HIP, std::string("upload failed") + sfx);
    if (ne > 0 && !p->tables &&
        (hipMemcpy(p->d_err, desc->err_terms, n_err_terms * sizeof(Term), hipMemcpyHostToDevice) != hipSuccess ||
         hipMemcpy(p->d_err_off, desc->err_term_offsets, ((size_t)ne + 1) * sizeof(int), hipMemcpyHostToDevice) !=
             hipSuccess))
        return fail(GRAPE_ERR_HIP, std::string("upload failed") + err_sfx);
    P.h0 = p->d_h0;
    P.tgt = p->d_tgt;
    P.vs = p->d_vs;
    P.err = p->d_err;
    P.err_off = p->d_err_off;
    return GRAPE_OK;
}

int create_dense(const grape_desc *desc, grape_plan *p, bool xadd_dep, const ProjectorSetup &ps, int n_err_terms) {
    const int D = desc->ndim, ne = desc->nerr;
    // H0 (or Herror) reading x_add: without error sources k_dgrad adds each step's x_add variant (DP.nva);
    // with error sources (round 6) the variant table carries the x_add variants too (the small engine's
    // layout: nvg = np + na gradient parameters per step), k_dlocal / k_derr_grad write their per-step x_add
    // terms and k_dadd sums them onto the target's parts (UnitaryCalculations.jl:57-64, 87-95)
    // Hermitian H0: checked for every engine in choose_route (the dense no-interchange
    // solve relies on it too, grape_dense.hpp).  The error variants exponentiate
    // H0 + err Herror (err <= eps2): Hermitian error terms keep them inside that proof.
    for (int e = 0; e < ne; ++e)  // (each source on its own: its terms' sum must be Hermitian)
        if (int rc = check_hermitian_terms(desc, desc->err_terms + desc->err_term_offsets[e],
                                           desc->err_term_offsets[e + 1] - desc->err_term_offsets[e],
                                           "error source (dense engine)"))
            return rc;
    if (grape_dense::set_lds_limits() != hipSuccess) return fail(GRAPE_ERR_HIP, "cannot raise LDS limit (dense)");
    p->dense = true;
    grape_dense::DenseProblem &DP = p->DP;
    DevProblem &P = DP.P;
    fill_problem_scalars(desc, ps.trP, P);
    // propagator variants (the small engine's layout, grape_plan_setup.hpp build_variants): nominal alone
    // without error sources (k_dgrad exponentiates its variants in place)
    const int nva = xadd_dep ? desc->nadd : 0, nvg = desc->nparam + nva;
    const std::vector<grape::VSpec> vs = set_variants(P, nva, ne > 0);
    P.nv = (int)vs.size();
    P.nvg = ne > 0 ? nvg : P.np;
    DP.nz = P.nvg * (1 + ne) + ne;
    P.nz = DP.nz;
    DP.nva = xadd_dep ? P.na : 0;
    // scan chunking: ~sqrt(N_t) chunks balances the chunk chains against the carry chain
    int nc = (int)std::ceil(std::sqrt((double)P.Nt));
    DP.Lc = (P.Nt + nc - 1) / nc;
    DP.Nc = (P.Nt + DP.Lc - 1) / DP.Lc;
    const size_t IMG = grape_dense::kImgDoubles, MB = p->max_batch, NE = ne;
    std::vector<double> img((size_t)desc->n_ops * IMG), W(64, 0.0);
    for (int o = 0; o < desc->n_ops; ++o) to_dense_image(desc->ops + 2 * (size_t)o * D * D, D, img.data() + o * IMG);
    for (int i = 0; i < D; ++i) W[i] = ps.W[i];
    bool ok = p->mem.alloc(&p->dn_opimg, img.size()) == hipSuccess && p->mem.alloc(&p->dn_W, (size_t)64) == hipSuccess &&
              p->mem.alloc(&p->dn_E, MB * P.Nt * P.nv * IMG) == hipSuccess && p->mem.alloc(&p->dn_Q, MB * P.Nt * IMG) == hipSuccess &&
              p->mem.alloc(&p->dn_Carry, MB * DP.Nc * IMG) == hipSuccess && p->mem.alloc(&p->dn_M, MB * IMG) == hipSuccess &&
              p->mem.alloc(&p->dn_Mc, MB * DP.Nc * IMG) == hipSuccess &&
              p->mem.alloc(&p->dn_Z, ne ? 1 : MB * P.Nt * IMG) == hipSuccess &&
              p->mem.alloc(&p->d_x, MB * P.nx) == hipSuccess &&
              p->mem.alloc(&p->d_F, MB) == hipSuccess && p->mem.alloc(&p->d_Fdx, MB * P.nx) == hipSuccess &&
              p->mem.alloc(&p->d_ctrl, kCtrlInts) == hipSuccess;
    if (ok && DP.nva > 0) ok = p->mem.alloc(&p->dn_Fadd, MB * P.Nt * DP.nva) == hipSuccess;
    if (ok && DP.nva > 0 && ne > 0) ok = p->mem.alloc(&p->dn_Fd2add, MB * NE * P.Nt * DP.nva) == hipSuccess;
    if (ok && ne > 0)
        ok = p->mem.alloc(&p->dn_Ub, MB * IMG) == hipSuccess && p->mem.alloc(&p->dn_Zl, MB * P.Nt * DP.nz * IMG) == hipSuccess &&
             p->mem.alloc(&p->dn_Vc, MB * NE * DP.Nc * IMG) == hipSuccess &&
             p->mem.alloc(&p->dn_Sx, MB * NE * DP.Nc * IMG) == hipSuccess && p->mem.alloc(&p->dn_Tot, MB * NE * IMG) == hipSuccess &&
             p->mem.alloc(&p->dn_Me, MB * NE * IMG) == hipSuccess && p->mem.alloc(&p->dn_Mp, MB * NE * DP.Nc * IMG) == hipSuccess &&
             p->mem.alloc(&p->dn_B0, MB * NE * DP.Nc * IMG) == hipSuccess && p->mem.alloc(&p->d_Fd2, MB * NE) == hipSuccess &&
             p->mem.alloc(&p->d_Fd2dx, MB * NE * P.nx) == hipSuccess;
    if (ok && ps.general && ne == 0) ok = p->mem.alloc(&p->dn_Ub, MB * IMG) == hipSuccess;
    if (!ok) return fail(GRAPE_ERR_ALLOC, "device allocation failed (dense)");
    {  // row-major operator basis: the general-projector heads and the analysis kernels
        std::vector<cd> ops((size_t)desc->n_ops * D * D);
        grape_setup::to_tiles(desc->ops, desc->n_ops, D, nullptr, 1, D, ops.data(), nullptr);
        if (p->mem.alloc(&p->d_ops, ops.size()) != hipSuccess ||
            hipMemcpy(p->d_ops, ops.data(), ops.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess)
            return fail(GRAPE_ERR_ALLOC, "device allocation failed (dense, general projector)");
        P.ops = p->d_ops;
    }
    if (int rc = upload_projector(p, ps, P, MB * std::max<size_t>(NE, 1))) return rc;
    if (hipMemset(p->d_ctrl, 0, kCtrlInts * sizeof(int)) != hipSuccess ||
        hipMemcpy(p->dn_opimg, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->dn_W, W.data(), 64 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "upload failed (dense)");
    if (int rc = upload_terms(p, desc, n_err_terms, vs, P, " (dense)", " (dense error terms)")) return rc;
    DP.opimg = p->dn_opimg;
    DP.W = p->dn_W;
    P.W = p->dn_W;  // zero-padded to 64; the analysis kernels (expectation values) read W[0..D)
    p->P = P;  // the C ABI reads nx / np / ne from the plan's problem for every engine
    return GRAPE_OK;
}

// ---------------------------------------------------------------------------
// tiled engine plan (GRAPE_MAX_DENSE_DIM < d <= GRAPE_MAX_TILED_DIM; grape_tiled.hip)
// ---------------------------------------------------------------------------
// column-major interleaved d x d complex <-> zero-padded row-major planes (re, then im) of P x P
void to_tiled_image(const double *src, int d, double *img) {
    const int P = grape_tiled::padded_dim(d);
    const size_t plane = (size_t)P * P;
    std::fill(img, img + 2 * plane, 0.0);
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i) {
            img[(size_t)i * P + j] = src[2 * ((size_t)i + (size_t)j * d)];
            img[plane + (size_t)i * P + j] = src[2 * ((size_t)i + (size_t)j * d) + 1];
        }
}
void from_tiled_image(const double *img, int d, double *dst) {
    const int P = grape_tiled::padded_dim(d);
    const size_t plane = (size_t)P * P;
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i) {
            dst[2 * ((size_t)i + (size_t)j * d)] = img[(size_t)i * P + j];
            dst[2 * ((size_t)i + (size_t)j * d) + 1] = img[plane + (size_t)i * P + j];
        }
}

// A tiled plan's workspace is sized by bytes, not by max_batch x everything: a quarter of the budget (at most
// kTiledSlabItems items) holds the slab of the exponential and of the gradient's eps-variants, the rest the
// evaluations of one pass (E and Q: 2 N_t images each, 512 MB at P = 128, N_t = 1 024).  A call of more
// evaluations than fit runs as several passes with identical arithmetic.  With error sources the same budget
// also holds every step's local-frame images (grape_tiled_api.hpp err_eval_images: 1.25 GB more per evaluation
// at that size with np = 2, ne = 1) and np + 1 more images per slab item.
constexpr size_t kTiledBudgetBytes = (size_t)6 << 30;
constexpr size_t kTiledSlabItems = 1024;
constexpr size_t kTiledSlabImages = 9;  // A, A^2, A^3, A^4, two Horner buffers, E', Q_{k-1} M'_c, Y^dag

// slab of the exponential: `items` images in each of the six buffers, from one allocation
hipError_t alloc_exp_slab(DevicePool &mem, size_t items, size_t img, grape_tiled::ExpSlab &X,
                                 double **extra, size_t n_extra) {
    double *base = nullptr;
    const hipError_t e = mem.alloc(&base, (6 + n_extra) * items * img);
    if (e != hipSuccess) return e;
    X.slab = (int)items;
    double **slots[6] = {&X.A, &X.A2, &X.A3, &X.A4, &X.B0, &X.B1};
    for (int i = 0; i < 6; ++i) *slots[i] = base + (size_t)i * items * img;
    for (size_t i = 0; i < n_extra; ++i) extra[i] = base + (6 + i) * items * img;
    return hipSuccess;
}

int create_tiled(const grape_desc *desc, grape_plan *p, const ProjectorSetup &ps) {
    const int D = desc->ndim;
    p->tiled = true;
    grape_tiled::TiledProblem &TP = p->TP;
    DevProblem &P = TP.P;
    fill_problem_scalars(desc, ps.trP, P);
    // the nominal alone is kept; with error sources (GRAPE_OPT_TILED_ERR) the list is the dense engine's, and
    // launch_pipeline exponentiates its variants slab by slab into the local-frame images
    const int ne = desc->nerr;
    const std::vector<grape::VSpec> vs = set_variants(P, 0, ne > 0);
    P.nv = ne > 0 ? (int)vs.size() : 1;
    P.nvg = P.np;
    P.nz = ne > 0 ? P.np + ne + ne * P.np : 0;
    TP.Pd = grape_tiled::padded_dim(D);
    // scan chunking: ~sqrt(N_t) chunks, as the dense engine
    const int nc = (int)std::ceil(std::sqrt((double)P.Nt));
    TP.Lc = (P.Nt + nc - 1) / nc;
    TP.Nc = (P.Nt + TP.Lc - 1) / TP.Lc;
    const size_t IMG = grape_tiled::image_doubles(D), imgB = IMG * sizeof(double);
    const size_t Nt = P.Nt, Nc = TP.Nc, nh = 1 + (size_t)P.na;
    // error sources: the local-frame images of every step are stored (np + ne + ne np per step), not recomputed
    // from a second round of variant exponentials, and the slab holds the eps2-variants of its steps
    const size_t NE = ne, NP = P.np;
    const size_t eval_imgs = 2 * Nt + 3 * Nc + 4 + 2 * nh + grape_tiled::err_eval_images(Nt, Nc, NP, P.na, NE);
    const size_t slab_imgs = kTiledSlabImages + grape_tiled::err_slab_images(NP, NE);
    size_t slab = std::min<size_t>(kTiledSlabItems, std::max<size_t>(1, kTiledBudgetBytes / 4 / (slab_imgs * imgB)));
    slab = std::min(slab, (size_t)p->max_batch * Nt);
    const size_t slabB = slab * slab_imgs * imgB;
    const size_t fit = kTiledBudgetBytes > slabB ? (kTiledBudgetBytes - slabB) / (eval_imgs * imgB) : 0;
    if (fit < 1)
        return fail(GRAPE_ERR_ALLOC, "tiled engine: one evaluation needs " + std::to_string(eval_imgs * imgB + slabB) +
                                         " bytes of workspace, the plan's budget is " + std::to_string(kTiledBudgetBytes));
    p->max_batch = (int)std::min<size_t>(p->max_batch, fit);
    const size_t MB = p->max_batch;
    grape_tiled::TiledBatch &B = p->TB;
    double *opimg = nullptr, *W = nullptr, *extra[3] = {nullptr, nullptr, nullptr};
    bool ok = p->mem.alloc(&opimg, (size_t)desc->n_ops * IMG) == hipSuccess && p->mem.alloc(&W, (size_t)TP.Pd) == hipSuccess &&
              p->mem.alloc(&B.E, MB * Nt * IMG) == hipSuccess && p->mem.alloc(&B.Q, MB * Nt * IMG) == hipSuccess &&
              p->mem.alloc(&B.Carry, MB * Nc * IMG) == hipSuccess && p->mem.alloc(&B.Tm, MB * Nc * IMG) == hipSuccess &&
              p->mem.alloc(&B.Mc, MB * Nc * IMG) == hipSuccess && p->mem.alloc(&B.U, MB * IMG) == hipSuccess &&
              p->mem.alloc(&B.M, MB * IMG) == hipSuccess && p->mem.alloc(&B.WK, MB * IMG) == hipSuccess &&
              p->mem.alloc(&B.T, MB * IMG) == hipSuccess && p->mem.alloc(&B.U0, MB * nh * IMG) == hipSuccess &&
              p->mem.alloc(&B.K, MB * nh * IMG) == hipSuccess && p->mem.alloc(&B.tau, 2 * MB) == hipSuccess &&
              p->mem.alloc(&B.ctl, MB * Nt) == hipSuccess && p->mem.alloc(&B.smax, (size_t)1) == hipSuccess &&
              alloc_exp_slab(p->mem, slab, IMG, B.X, extra, 3) == hipSuccess &&
              p->mem.alloc(&p->d_x, MB * P.nx) == hipSuccess && p->mem.alloc(&p->d_F, MB) == hipSuccess &&
              p->mem.alloc(&p->d_Fdx, MB * P.nx) == hipSuccess && p->mem.alloc(&p->d_ctrl, kCtrlInts) == hipSuccess;
    if (ok && ne > 0) {
        const size_t bec = MB * NE * Nc * IMG, be = MB * NE * IMG;
        double **per_chunk[10] = {&B.Sd, &B.Tmp, &B.Vc, &B.Sx, &B.Dx, &B.Mce, &B.Tce, &B.Dce, &B.Bst, &B.Lam};
        double **per_src[5] = {&B.Tot, &B.Ue, &B.UeU, &B.KW, &B.Me};
        for (double **q : per_chunk) ok = ok && p->mem.alloc(q, bec) == hipSuccess;
        for (double **q : per_src) ok = ok && p->mem.alloc(q, be) == hipSuccess;
        ok = ok && p->mem.alloc(&B.Zl, MB * Nt * (size_t)P.nz * IMG) == hipSuccess &&
             p->mem.alloc(&B.Ke, be * nh) == hipSuccess && p->mem.alloc(&B.taue, 2 * MB * NE) == hipSuccess &&
             p->mem.alloc(&B.Eh, (NP + 1) * slab * IMG) == hipSuccess && p->mem.alloc(&p->d_Fd2, MB * NE) == hipSuccess && p->mem.alloc(&p->d_Fd2dx, MB * NE * P.nx) == hipSuccess;
    }
    if (!ok) return fail(GRAPE_ERR_ALLOC, "device allocation failed (tiled)");
    B.Ev = extra[0];
    B.Ts = extra[1];
    B.Yd = extra[2];
    if (hipHostMalloc(reinterpret_cast<void **>(&p->tl_h_smax), sizeof(int), hipHostMallocDefault) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "pinned allocation failed (tiled)");
    B.h_smax = p->tl_h_smax;
    std::vector<double> img((size_t)desc->n_ops * IMG), Wp(TP.Pd, 0.0);
    for (int o = 0; o < desc->n_ops; ++o) to_tiled_image(desc->ops + 2 * (size_t)o * D * D, D, img.data() + o * IMG);
    for (int i = 0; i < D; ++i) Wp[i] = ps.W[i];
    if (hipMemset(p->d_ctrl, 0, kCtrlInts * sizeof(int)) != hipSuccess ||
        hipMemcpy(opimg, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(W, Wp.data(), Wp.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "upload failed (tiled)");
    if (int rc = upload_terms(p, desc, ne > 0 ? desc->err_term_offsets[ne] : 0, vs, P, " (tiled)", " (tiled error terms)"))
        return rc;
    TP.opimg = opimg;
    TP.W = W;
    P.W = W;
    p->P = P;  // the C ABI reads nx / np / ne from the plan's problem for every engine
    return GRAPE_OK;
}

// ---------------------------------------------------------------------------
// plan creation, phase by phase (grape_plan_create calls them top to bottom; each returns a GRAPE_*
// code with the message set, and the caller frees the plan on any failure)
// ---------------------------------------------------------------------------
// the factor slots on the plan's device
int upload_factors(grape_plan *p, const FactorSplit &fs) {
    if (!fs.any) return GRAPE_OK;
    if (p->mem.alloc(&p->d_fac_h0, fs.fac_h0.size()) != hipSuccess || p->mem.alloc(&p->d_fac_err, fs.fac_err.size()) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (product factors)");
    if (hipMemcpy(p->d_fac_h0, fs.fac_h0.data(), fs.fac_h0.size() * sizeof(Term), hipMemcpyHostToDevice) != hipSuccess ||
        (!fs.fac_err.empty() &&
         hipMemcpy(p->d_fac_err, fs.fac_err.data(), fs.fac_err.size() * sizeof(Term), hipMemcpyHostToDevice) != hipSuccess))
        return fail(GRAPE_ERR_HIP, "upload failed (product factors)");
    p->FT.h0 = p->d_fac_h0;
    p->FT.err = p->d_fac_err;
    return GRAPE_OK;
}

// the plan's device, stream and pinned status word
int open_plan(grape_plan *p, const grape_desc *desc, int device, const Route &rt) {
    for (int k = 0; k < (rt.tables ? 0 : desc->n_h0_terms); ++k)
        if (desc->h0_terms[k].var == GRAPE_VAR_TSTEP) p->uses_tstep = true;
    p->device = device;
    p->max_batch = desc->max_batch > 0 ? desc->max_batch : 256;
    p->pivot = rt.pivot;
    if (hipSetDevice(device) != hipSuccess) return fail(GRAPE_ERR_HIP, "hipSetDevice failed");
    if (hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "hipStreamCreate failed");
    p->stream = p->own_stream;
    if (hipHostMalloc(reinterpret_cast<void **>(&p->h_status), sizeof(int), hipHostMallocDefault) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "pinned allocation failed");
    *p->h_status = 0;
    return GRAPE_OK;
}

// The whole-matrix problem P: scalars, variant layout, scan chunking; then the sector layout (host).
static int setup_problem(PlanBuild &b) {
    const grape_desc *desc = b.desc;
    grape_plan *p = b.p;
    const int D = desc->ndim;
    if (D <= GRAPE_MAX_SMALL_DIM && dispatch_lds_limits(D) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "cannot raise LDS limit");
    DevProblem &P = p->P;
    p->tables = b.rt.tables;
    p->general_h0 = b.rt.general_h0;
    b.n_ops = b.rt.tables ? 0 : desc->n_ops;
    fill_problem_scalars(desc, b.ps.trP, P);
    P.xadd_dep = b.rt.xadd_dep ? 1 : 0;
    // propagator variants of one step (grape_plan_setup.hpp build_variants), with the x_add variants
    // only if H0 reads x_add
    const int nad = b.rt.xadd_dep ? desc->nadd : 0;
    b.vs = set_variants(P, nad, true);
    // E stores every variant for the error-source pipeline; without error sources
    // only the nominal propagators are stored (k_expm_grad consumes the rest in place)
    // host tables: every variant's propagator is stored (k_grad reads them back)
    P.nv = (desc->nerr > 0 || b.rt.tables) ? (int)b.vs.size() : 1;
    P.nvg = desc->nparam + nad;
    P.nz = P.nvg * (1 + desc->nerr) + desc->nerr;
    // scan width: narrow once a launch can hold two evaluations per CU
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, p->device) == hipSuccess && prop.multiProcessorCount > 0)
        b.ncu = prop.multiProcessorCount;
    b.scan_override = desc->reserved[2];
    P.scan_waves = p->max_batch >= 2 * b.ncu ? kScanNarrow : kScanWide;
    if (b.scan_override == kScanNarrow || b.scan_override == kScanWide) P.scan_waves = b.scan_override;
    const int nc0 = std::min(P.scan_waves * (64 / D), P.Nt);
    P.L = (P.Nt + nc0 - 1) / nc0;
    P.nchunks = (P.Nt + P.L - 1) / P.L;
    P.sectors = 0;
    P.nsec = 1;
    P.sec_ops = 0;
    // symmetry-adapted sectors: the sector path (operators, head) in the rotated basis when that
    // splits the sectors further; the whole-matrix problem P keeps the caller's basis
    if (!b.rt.general_h0 && !b.rt.tables) b.sym = symmetry_setup(desc);
    b.sdesc = b.sym.on ? b.sym.view(desc) : *desc;
    if (!b.rt.general_h0) {
        const std::vector<char> idle = b.rt.tables ? std::vector<char>() : idle_levels(desc, b.sdesc, b.sps());
        b.ss = find_sectors(&b.sdesc, b.rt.tables, b.rt.tables ? nullptr : &idle);
    }
    p->symmetry = b.sym.on;
    return GRAPE_OK;
}

// The whole-matrix workspace (no rows when sectors or the general-H0 path run), the per-call buffers
// every path uses, and the uploads of operators, terms, weights and projector.
static int alloc_whole_matrix(PlanBuild &b) {
    const grape_desc *desc = b.desc;
    grape_plan *p = b.p;
    DevProblem &P = p->P;
    const bool tables = b.rt.tables;
    const int D = P.D;
    const size_t FR = (!b.ss.cls.empty() || b.rt.general_h0) ? 0 : (size_t)p->max_batch;
    const size_t MB = p->max_batch, T = (size_t)D * D;
    std::vector<cd> ops((size_t)b.n_ops * T), opsT(ops.size());
    grape_setup::to_tiles(desc->ops, b.n_ops, D, nullptr, 1, D, ops.data(), opsT.data());
    bool ok = p->mem.alloc(&p->d_ops, ops.size()) == hipSuccess && p->mem.alloc(&p->d_opsT, opsT.size()) == hipSuccess &&
              p->mem.alloc(&p->d_W, (size_t)D) == hipSuccess &&
              p->mem.alloc(&p->d_E, FR * P.Nt * P.nv * T) == hipSuccess && p->mem.alloc(&p->d_Q, FR * P.Nt * T) == hipSuccess &&
              p->mem.alloc(&p->d_Mc, FR * P.nchunks * T) == hipSuccess && p->mem.alloc(&p->d_x, MB * P.nx) == hipSuccess &&
              p->mem.alloc(&p->d_F, MB) == hipSuccess && p->mem.alloc(&p->d_Fdx, MB * P.nx) == hipSuccess &&
              p->mem.alloc(&p->d_part, MB * P.Nt * std::max(P.na, 1)) == hipSuccess &&
              p->mem.alloc(&p->d_tgt_part, MB * std::max(P.na, 1)) == hipSuccess &&
              p->mem.alloc(&p->d_ovf, FR * P.Nt * P.nv) == hipSuccess && p->mem.alloc(&p->d_ctrl, kCtrlInts) == hipSuccess &&
              p->mem.alloc(&p->d_sink, T) == hipSuccess;
    if (ok && P.ne == 0)
        ok = p->mem.alloc(&p->d_ovf2, FR * P.Nt * P.nvg) == hipSuccess &&
             p->mem.alloc(&p->d_ovf2_slots, FR * P.Nt * P.nvg * T) == hipSuccess;
    if (ok && (P.ne > 0 || b.ps.general))  // carries and U: the error path and the general-projector heads
        ok = p->mem.alloc(&p->d_Carry, FR * P.nchunks * T) == hipSuccess && p->mem.alloc(&p->d_Ub, FR * T) == hipSuccess;
    if (ok && P.ne > 0)
        ok = p->mem.alloc(&p->d_Me, FR * P.ne * P.nchunks * 3 * T) == hipSuccess &&
             p->mem.alloc(&p->d_Fd2, MB * P.ne) == hipSuccess && p->mem.alloc(&p->d_Fd2dx, MB * P.ne * P.nx) == hipSuccess &&
             p->mem.alloc(&p->d_Zl, FR * P.Nt * P.nz * T) == hipSuccess;
    if (ok && P.ne > 0 && P.xadd_dep)
        ok = p->mem.alloc(&p->d_part_err, MB * P.ne * P.Nt * P.na) == hipSuccess;
    if (ok && tables)
        ok = p->mem.alloc(&p->d_Htab, MB * P.Nt * P.nv * T) == hipSuccess &&
             p->mem.alloc(&p->d_U0tab, MB * (1 + P.na) * T) == hipSuccess;
    if (!ok) return fail(GRAPE_ERR_ALLOC, "device allocation failed");
    if (hipMemset(p->d_ctrl, 0, kCtrlInts * sizeof(int)) != hipSuccess) return fail(GRAPE_ERR_HIP, "memset failed");
    if (int rc = upload_terms(p, desc, b.n_err_terms, b.vs, P, "", "")) return rc;
    if ((!tables &&
         (hipMemcpy(p->d_ops, ops.data(), ops.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(p->d_opsT, opsT.data(), opsT.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess)) ||
        hipMemcpy(p->d_W, b.ps.W.data(), D * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "upload failed");
    if (int rc = upload_projector(p, b.ps, P, MB * std::max(P.ne, 1))) return rc;
    P.ops = p->d_ops;
    P.opsT = p->d_opsT;
    P.W = p->d_W;
    return GRAPE_OK;
}

// a diagonal projector's tiles A = diag(w), B = diag(w != 0) (or the given general ones) on the device
static hipError_t upload_projector_tiles(grape_plan *p, const std::vector<cd> &A, const std::vector<cd> &B, cd **dA, cd **dB) {
    hipError_t e = p->mem.alloc(dA, A.size());
    if (e == hipSuccess) e = p->mem.alloc(dB, B.size());
    if (e == hipSuccess) e = hipMemcpy(*dA, A.data(), A.size() * sizeof(cd), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(*dB, B.data(), B.size() * sizeof(cd), hipMemcpyHostToDevice);
    return e;
}

// General H0: the fidelity heads need P0 P and P as tiles; the chain's inverses and the head's scratch.
static int setup_general_h0(PlanBuild &b) {
    if (!b.rt.general_h0) return GRAPE_OK;
    grape_plan *p = b.p;
    DevProblem &P = p->P;
    const size_t T = (size_t)P.D * P.D;
    if (!b.ps.general) {
        std::vector<cd> A, Bm;
        grape_setup::diag_projector_tiles(b.ps.W.data(), P.D, A, Bm);
        if (upload_projector_tiles(p, A, Bm, &p->d_PA, &p->d_PB) != hipSuccess)
            return fail(GRAPE_ERR_ALLOC, "device allocation failed (general H0)");
        P.PA = p->d_PA;
        P.PB = p->d_PB;
    }
    if (p->mem.alloc(&p->ud_Ci, (size_t)P.Nt * T) != hipSuccess || p->mem.alloc(&p->d_G, (1 + (size_t)P.ne) * T) != hipSuccess ||
        (P.D > grape_unitary::kMaxD && p->mem.alloc(&p->d_fscr, (size_t)grape_unitary::kFidTiles * T) != hipSuccess))
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (general H0)");
    return GRAPE_OK;
}

// The head over the assembled U (SH): its projector tiles, weights and operators (the rotated ones
// with symmetry-adapted sectors), the fixed levels, and the choice of the diagonal head.
static int setup_sector_head(PlanBuild &b) {
    const grape_desc *desc = b.desc;
    grape_plan *p = b.p;
    const DevProblem &P = p->P;
    const ProjectorSetup &sps = b.sps();
    const SectorSetup &ss = b.ss;
    const bool sym = b.sym.on;
    const int D = P.D;
    std::vector<cd> A, Bm;
    grape_setup::diag_projector_tiles(sps.W.data(), D, A, Bm);
    if (sym && sps.general) {
        A = sps.A;
        Bm = sps.B;
    }
    if (sym) {  // the head's own rotated projector tiles, weights and operators
        std::vector<cd> rops((size_t)b.n_ops * D * D), ropsT(rops.size());
        grape_setup::to_tiles(b.sym.ops.data(), b.n_ops, D, nullptr, 1, D, rops.data(), ropsT.data());
        if (upload_projector_tiles(p, A, Bm, &p->d_PA_sym, &p->d_PB_sym) != hipSuccess ||
            p->mem.alloc(&p->d_W_sym, (size_t)D) != hipSuccess || p->mem.alloc(&p->d_ops_sym, rops.size()) != hipSuccess ||
            p->mem.alloc(&p->d_opsT_sym, ropsT.size()) != hipSuccess ||
            hipMemcpy(p->d_W_sym, sps.W.data(), D * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(p->d_ops_sym, rops.data(), rops.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(p->d_opsT_sym, ropsT.data(), ropsT.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess)
            return fail(GRAPE_ERR_ALLOC, "device allocation failed (symmetry sectors)");
    } else if (!b.ps.general && upload_projector_tiles(p, A, Bm, &p->d_PA, &p->d_PB) != hipSuccess) {
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (sectors)");
    }
    if (p->mem.alloc(&p->d_fixed, ss.fixed.size()) != hipSuccess ||
        (!ss.fixed.empty() && hipMemcpy(p->d_fixed, ss.fixed.data(), ss.fixed.size() * sizeof(int),
                                        hipMemcpyHostToDevice) != hipSuccess))
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (sectors)");
    grape_proj::SectorHead &H = p->SH;
    H.P = P;
    H.P.PA = sym ? p->d_PA_sym : p->d_PA;
    H.P.PB = sym ? p->d_PB_sym : p->d_PB;
    if (sym) {
        H.P.W = p->d_W_sym;
        H.P.ops = p->d_ops_sym;
        H.P.opsT = p->d_opsT_sym;
    }
    H.ncls = (int)ss.cls.size();
    H.fixed = p->d_fixed;
    H.nfixed = (int)ss.fixed.size();
    // diagonal projector and target, classes of <= 4 levels, at most kDiagMaxRows sector rows: the
    // row-parallel heads (grape_projector.hip k_sec_head_diag, k_sec_err_head_rows)
    H.diag = !sps.general && !b.rt.tables && !(P.opts & GRAPE_OPT_GENERAL_HEAD);
    int rows = 0;  // the heads' lanes per evaluation (grape_projector.hip diag_group)
    for (const SectorClass &sc : ss.cls) {
        H.diag = H.diag && sc.S <= 4;
        rows += sc.nsec * sc.S;
    }
    H.diag = H.diag && rows <= grape_proj::kDiagMaxRows;
    for (int k = 0; H.diag && k < desc->n_target_terms; ++k) {
        const double *op = b.sdesc.ops + 2 * (size_t)desc->target_terms[k].op * D * D;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j)
                if (i != j && (op[2 * (i + (size_t)j * D)] != 0.0 || op[2 * (i + (size_t)j * D) + 1] != 0.0))
                    H.diag = 0;
    }
    return GRAPE_OK;
}

// Every decision about one sector class, into Ps (pure host logic; gauge_n: the class's charges, for
// alloc_class to upload; sops: the class's operator tiles [w][o][S][S]).
static void decide_class(const PlanBuild &b, const SectorClass &sc, const std::vector<cd> &sops, DevProblem &Ps,
                         std::vector<int> &gauge_n) {
    const grape_desc *desc = b.desc;
    const DevProblem &P = b.p->P;
    const int S = sc.S, ncu = b.ncu, scan_override = b.scan_override;
    const size_t TS = (size_t)S * S, MB = b.p->max_batch, R = MB * sc.nsec;  // workspace rows: sub-evaluations
    Ps = P;
    Ps.D = S;
    Ps.sectors = 1;
    Ps.nsec = sc.nsec;
    Ps.sec_ops = (size_t)b.n_ops * TS;
    Ps.gen_proj = 0;
    Ps.scan_waves = (long)R >= 8L * ncu ? kScanTiny : (long)R >= 2L * ncu ? kScanNarrow : kScanWide;
    if (scan_override == kScanTiny || scan_override == kScanNarrow || scan_override == kScanWide)
        Ps.scan_waves = scan_override;
    // chunk walks (grape_walk.hpp): classes of <= kWalkMaxD levels; with error sources the
    // image walk (k_walk_img), for any number of gradient parameters per step
    // (its exponential keeps A skew-Hermitian in compressed form: Hermitian error generators only;
    // a decay-rate error, -i e/2 |r><r|, keeps the stored-variant kernels)
    Ps.walk = (S <= grape::kWalkMaxD && (P.ne == 0 || b.rt.err_herm) && P.np <= grape::kWalkMaxNpA &&
               P.na <= grape::kWalkMaxNpA && !(P.opts & GRAPE_OPT_NO_WALK)) ? 1 : 0;
    // phase-covariant classes (grape_walk.hpp GAUGE): one exponential per walk lane
    // (with error sources: the phase-covariant image walk, one gradient parameter per step)
    double gauge_a = 1.0;
    Ps.gauge = (Ps.walk && (P.ne == 0 || (P.nvg == 1 && P.ne <= grape::kGaugeMaxE)) &&
                !(P.opts & GRAPE_OPT_NO_GAUGE) && find_gauge(desc, b.sdesc, sc, gauge_a, gauge_n)) ? 1 : 0;
    Ps.gauge_a = gauge_a;
    Ps.gauge_n = nullptr;
    Ps.gauge_ladder = Ps.gauge;
    for (size_t i = 0; Ps.gauge && i < gauge_n.size(); ++i)
        if (gauge_n[i] != (int)(i % (size_t)S)) Ps.gauge_ladder = 0;
    // error sources on a phase-covariant class: the lab-frame walks (no images, grape_walk.hpp,
    // GRAPE_WALK_ERR_LAB) when the base table's lanes fit one workgroup
    Ps.gauge_lab = (GRAPE_WALK_ERR_LAB && Ps.gauge && P.ne > 0 &&
                    sc.nsec * (1 + 2 * P.ne) <= grape::kLabBaseMaxLanes) ? 1 : 0;
    Ps.gauge_Et = nullptr;
    // the forward walk hands its propagators to the gradient walk (HBM, lane-minor) where the
    // exponential is the expensive part: the 4-level class (grape_walk.hpp; measured C2 6.04 ->
    // 6.52 M evals/s; for the 2-level class it lost, 0.72 -> 1.01 ms per pass)
    Ps.walk_store_e = Ps.walk && !Ps.gauge && P.ne == 0 && S >= grape::kWalkStoreMinD &&
                      !(P.opts & GRAPE_OPT_WALK_RECOMPUTE) ? 1 : 0;
    // latency-bound walk classes (fewer sub-evaluations than CUs, or the option): 16-wave scans,
    // half-length walks (grape_launch.hpp kScanLatency)
    // (not the error walks: the longer error scans cost more than the shorter walks save)
    if (Ps.walk && P.ne == 0 &&
        (scan_override == kScanLatency || (scan_override == 0 && (long)R < (long)ncu)))
        Ps.scan_waves = kScanLatency;
    // phase-covariant throughput classes: a step costs a few products instead of an
    // exponential, so longer chunks (fewer per-lane prologues and a shorter scan) can pay
    const int cdiv = (Ps.gauge && Ps.scan_waves == kScanTiny) ? GRAPE_GAUGE_CHUNK_DIV : 1;
    int ncs = std::max(1, std::min(Ps.scan_waves * (64 / S) / cdiv, P.Nt));
    if (Ps.gauge && Ps.scan_waves == kScanTiny && S == 3 && P.ne == 0)
        ncs = merged_chunk_count((long)MB, P.Nt, ncs, ncu);
    // the lab-frame error walks' throughput chunking (A/B knobs; 0: the formula above)
    if (Ps.gauge_lab && Ps.scan_waves == kScanTiny) {
        const int lc = S >= 4 ? GRAPE_LAB_CHUNKS4 : GRAPE_LAB_CHUNKS2;
        if (lc > 0) ncs = std::max(1, std::min(lc, P.Nt));
    }
    Ps.L = (P.Nt + ncs - 1) / ncs;
    Ps.nchunks = (P.Nt + Ps.L - 1) / Ps.L;
    // twin sectors (grape_walk.hpp TWIN): two walk sectors whose blocks of every operator H0
    // and the error sources use are identical, with the same padding -- one exponential
    // per step serves both (the 2-level Rydberg sectors at equal Rabi frequencies)
    Ps.twin = 0;
    // (S == 2 only: launch<2> is the one launcher that runs a class with two sectors per lane)
    if (Ps.walk && P.ne == 0 && sc.nsec == 2 && S == 2 && !Ps.walk_store_e && !(P.opts & GRAPE_OPT_NO_TWIN)) {
        bool same = true;
        for (int a = 0; a < S; ++a) same = same && ((sc.sidx[a] < 0) == (sc.sidx[S + a] < 0));
        std::vector<char> used(b.n_ops, 0);
        for (int t = 0; t < desc->n_h0_terms; ++t) used[desc->h0_terms[t].op] = 1;
        for (int o = 0; same && o < b.n_ops; ++o)
            if (used[o])
                same = std::memcmp(&sops[(size_t)o * TS], &sops[((size_t)b.n_ops + o) * TS], TS * sizeof(cd)) == 0;
        Ps.twin = same ? 1 : 0;
    }
}

// The workspace of one sector class (sb[cl]) as decide_class sized it, and the uploads of its
// charges, operator tiles and level indices.
static int alloc_class(PlanBuild &b, int cl, const std::vector<int> &gauge_n, const std::vector<cd> &sops,
                       const std::vector<cd> &sopsT) {
    grape_plan *p = b.p;
    const DevProblem &P = p->P;
    DevProblem &Ps = p->Ps[cl];
    const SectorClass &sc = b.ss.cls[cl];
    grape_plan::SecBuf &sb = p->sb[cl];
    const size_t TS = (size_t)sc.S * sc.S, MB = p->max_batch, R = MB * sc.nsec, nvg = P.nvg;
    if (Ps.gauge) {
        if (p->mem.alloc(&sb.gauge_n, gauge_n.size()) != hipSuccess) return fail(GRAPE_ERR_ALLOC, "device allocation failed (gauge)");
        if (hipMemcpy(sb.gauge_n, gauge_n.data(), gauge_n.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
            return fail(GRAPE_ERR_HIP, "upload failed (gauge)");
        Ps.gauge_n = sb.gauge_n;
    }
    const size_t ne = (size_t)P.ne, R2 = (P.ne > 0 || Ps.walk) ? 0 : R;  // k_expm_grad parking: no error sources only
    const size_t RE = Ps.walk ? 0 : R;  // the walks store no E / Q
    const size_t lanes_pad = (MB * Ps.nchunks + grape::kWalkBlockA - 1) / grape::kWalkBlockA * grape::kWalkBlockA;
    // stored propagators: D*D elements + the diagonal shift per (step, sector) (grape_walk.hpp kEwStride)
    if (Ps.walk_store_e && p->mem.alloc(&sb.Ew, (size_t)sc.nsec * Ps.L * (TS + 1) * lanes_pad) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (sector walks)");
    if (Ps.walk && (p->mem.alloc(&sb.Tc, R * Ps.nchunks * TS) != hipSuccess ||
                    p->mem.alloc(&sb.wscr, 2 * (size_t)sc.nsec * lanes_pad * TS) != hipSuccess))
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (sector walks)");
    if (p->mem.alloc(&sb.E, RE * P.Nt * P.nv * TS) != hipSuccess || p->mem.alloc(&sb.Q, RE * P.Nt * TS) != hipSuccess ||
        p->mem.alloc(&sb.Mc, R * Ps.nchunks * TS) != hipSuccess || p->mem.alloc(&sb.Carry, R * Ps.nchunks * TS) != hipSuccess ||
        p->mem.alloc(&sb.Ub, R * TS) != hipSuccess || p->mem.alloc(&sb.Msec, R * TS) != hipSuccess ||
        p->mem.alloc(&sb.slots, R2 * P.Nt * nvg * TS) != hipSuccess || p->mem.alloc(&sb.ovf, RE * P.Nt * P.nv) != hipSuccess ||
        p->mem.alloc(&sb.ovf2, R2 * P.Nt * nvg) != hipSuccess || p->mem.alloc(&sb.part, R * P.Nt * nvg) != hipSuccess ||
        p->mem.alloc(&sb.sidx, sc.sidx.size()) != hipSuccess || p->mem.alloc(&sb.ops, sops.size()) != hipSuccess ||
        p->mem.alloc(&sb.opsT, sopsT.size()) != hipSuccess ||
        // (the image walk's images are lane-minor over its padded launch width: grape_walk.hpp img_index)
        p->mem.alloc(&sb.Zl, (Ps.walk ? (size_t)sc.nsec * Ps.L * lanes_pad : R * P.Nt) * (ne && !Ps.gauge_lab ? P.nz : 0) * TS) != hipSuccess ||
        p->mem.alloc(&sb.Wc, (Ps.walk ? R * ne * Ps.nchunks : 0) * TS) != hipSuccess ||
        p->mem.alloc(&sb.Me, R * ne * Ps.nchunks * 3 * TS) != hipSuccess || p->mem.alloc(&sb.TotS, R * ne * TS) != hipSuccess ||
        p->mem.alloc(&sb.MsecE, R * ne * TS) != hipSuccess || p->mem.alloc(&sb.part_err, R * ne * P.Nt * nvg) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (sectors)");
    if (hipMemcpy(sb.ops, sops.data(), sops.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(sb.opsT, sopsT.data(), sopsT.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(sb.sidx, sc.sidx.data(), sc.sidx.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "upload failed (sectors)");
    Ps.ops = sb.ops;
    Ps.opsT = sb.opsT;
    return GRAPE_OK;
}

// E~ of every sector of a phase-covariant class, once per plan, into sb[cl].gEt: the merged walks' table
// (grape_walk.hpp gauge_prop_lds: the walks' own exponential, so the same bits as a per-workgroup
// copy) or, err: the lab-frame error walks' base table (1 + 2 ne matrices per sector).
static int fill_gauge_table(grape_plan *p, int cl, bool err) {
    DevProblem &Pc = p->Ps[cl];
    const size_t nbm = (size_t)Pc.nsec * (err ? 1 + 2 * Pc.ne : 1), TS = (size_t)Pc.D * Pc.D;
    DevicePool tmp;  // the fill's scratch
    cd *scr = nullptr, *&gEt = p->sb[cl].gEt;
    if (p->mem.alloc(&gEt, nbm * TS) != hipSuccess || tmp.alloc(&scr, nbm * 2 * TS) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, err ? "device allocation failed (gauge error base)" : "device allocation failed (gauge base)");
    const hipError_t e = err ? grape_walk::fill_gauge_err_base(Pc, Pc.nsec, scr, gEt, p->stream)
                             : grape_walk::fill_gauge_base(Pc, Pc.nsec, scr, gEt, p->stream);
    const hipError_t es = hipStreamSynchronize(p->stream);
    if (e != hipSuccess || es != hipSuccess)
        return fail(GRAPE_ERR_HIP, err ? "gauge error base fill failed" : "gauge base fill failed");
    Pc.gauge_Et = gEt;
    return GRAPE_OK;
}

// The two walk classes of the Rydberg layout in the pair kernels' order: pa the 4- (or 3-) level
// class, pb the 2-level one.
void walk_pair_order(const grape_plan *p, int *pa, int *pb) {
    *pa = 0;
    *pb = 1;
    if (p->ncls == 2 && grape_walk::pair_ok(p->Ps[1], p->Ps[0])) std::swap(*pa, *pb);
}

// throughput passes of the Rydberg layout with phase-covariant classes: class B (2 levels)
// takes class A's chunking (fewer, longer chunks: its buffers, sized for its own count,
// suffice) so that one lane can walk both (merged walks; GRAPE_OPT_NO_MERGE launches the
// same chunking per class)
static int setup_merge(PlanBuild &b) {
    grape_plan *p = b.p;
    if (p->ncls != 2) return GRAPE_OK;
    const DevProblem &P = p->P;
    int pa, pb;
    walk_pair_order(p, &pa, &pb);
    DevProblem &A = p->Ps[pa], &Bq = p->Ps[pb];
    if (!(grape_walk::pair_ok(A, Bq) && A.D == 3 && A.gauge && Bq.gauge && A.gauge_a == Bq.gauge_a &&
          A.scan_waves == kScanTiny && Bq.scan_waves == kScanTiny && A.nchunks <= Bq.nchunks && P.np == 1 && P.na <= 1))
        return GRAPE_OK;
    Bq.L = A.L;
    Bq.nchunks = A.nchunks;
    p->merged = !(P.opts & GRAPE_OPT_NO_MERGE) && grape_walk::merged_ok(A, Bq);
    p->merge_pa = pa;
    for (int cl = 0; p->merged && cl < 2; ++cl)  // E~ of both classes for the merged walks' scalar loads
        if (int rc = fill_gauge_table(p, cl, false)) return rc;
    // The rank-one gradient walk (grape_walk.hpp merged_step_grad_r1, GRAPE_OPT_NO_RANK1): the diagonal head
    // writes row r of a sector's M block with the factor W[g_r] (grape_projector.hip diag_row, pass 1), so a
    // sector with exactly one weighted level (the head's W and level order: the rotated ones with
    // symmetry-adapted sectors) has M = e_c m^T.  Every sector of both classes must be such, and summed twins
    // must hold that level at one in-sector index; anything else keeps the matrix walk.
    const std::vector<double> &W = b.sps().W;
    bool r1 = p->merged && p->SH.diag && !(P.opts & GRAPE_OPT_NO_RANK1);
    for (int cl = 0; cl < 2; ++cl) {
        const SectorClass &sc = b.ss.cls[cl];
        DevProblem &Pc = p->Ps[cl];
        Pc.rank1 = Pc.rank1_c[0] = Pc.rank1_c[1] = 0;
        r1 = r1 && sc.nsec <= 2;
        for (int w = 0; r1 && w < sc.nsec; ++w) {
            int n = 0;
            for (int r = 0; r < sc.S; ++r) {
                const int g = sc.sidx[(size_t)w * sc.S + r];
                if (g >= 0 && W[g] != 0.0) {
                    Pc.rank1_c[w] = r;
                    p->wide_lev[cl][w] = g;
                    ++n;
                }
            }
            r1 = r1 && n == 1;
        }
        if (Pc.twin && grape_walk::merged_twin_sum()) r1 = r1 && Pc.rank1_c[0] == Pc.rank1_c[1];
    }
    A.rank1 = Bq.rank1 = r1 ? 1 : 0;
    // the wide pass: its U blocks and alphas take the chunk totals' and carries' buffers (alloc_class: at least
    // max_batch x nchunks tiles per sector of either class, class B's sized for its own, larger, chunk count)
    const long wide = (long)p->max_batch * A.nchunks;
    // (wide_ok and r1 give the wide head, k_wide_head, what it relies on: na <= 1, no x_add in H0, no error sources,
    // one weighted level per sector, 1 + 2 sectors; d <= 12 leaves at most kWideHeadMaxFixed untouched levels)
    if (r1 && !(P.opts & GRAPE_OPT_NO_WIDE) && grape_walk::wide_ok(A, Bq) && wide * 2 <= (long)INT_MAX &&
        p->SH.nfixed <= grape_proj::kWideHeadMaxFixed)
        p->wide = (int)wide;
    return GRAPE_OK;
}

// latency-bound calls of the Rydberg layout with phase-covariant classes: one workgroup per
// evaluation (grape_eval1.hip), with E~ of each class computed here once
static int setup_eval1(grape_plan *p) {
    const grape_proj::SectorHead &H = p->SH;
    if (p->ncls != 2 || (long)p->max_batch > kEval1MaxBatch || (p->P.opts & GRAPE_OPT_NO_EVAL1)) return GRAPE_OK;
    int pa, pb;
    walk_pair_order(p, &pa, &pb);
    const DevProblem &A = p->Ps[pa], &Bq = p->Ps[pb];
    if (!grape_walk::pair_ok(A, Bq) || !grape_eval1::eligible(A, Bq, H)) return GRAPE_OK;
    if (p->mem.alloc(&p->d_e1_Et, (size_t)A.D * A.D + 8) != hipSuccess ||
        p->mem.alloc(&p->d_e1_scr, (size_t)2 * 2 * 16) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (eval1)");
    const hipError_t e = grape_eval1::prepare(A, Bq, p->d_e1_Et, p->d_e1_Et + (size_t)A.D * A.D, p->d_e1_scr, p->stream);
    if (e != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "eval1 preparation failed");
    p->e1 = true;
    p->e1_pa = pa;
    const size_t tb = grape_eval1::tab_bytes(A, Bq, H);
    if (p->mem.alloc(&p->d_e1_tab, std::max<size_t>(tb, 16)) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (eval1)");
    if (grape_eval1::tab_build(eval1_args(p, nullptr, nullptr, nullptr), p->d_e1_tab, p->stream) != hipSuccess ||
        hipStreamSynchronize(p->stream) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "eval1 table build failed");
    const char *tr = std::getenv("GRAPE_EVAL1_TRACE");
    if (tr && tr[0] == '1' &&
        (hipHostMalloc(reinterpret_cast<void **>(&p->e1_trace), 32 * sizeof(long long), hipHostMallocDefault) != hipSuccess ||
         hipHostGetDevicePointer(reinterpret_cast<void **>(&p->e1_trace_d), p->e1_trace, 0) != hipSuccess))
        return fail(GRAPE_ERR_ALLOC, "eval1 trace buffer");
    return GRAPE_OK;
}

// The sector problems of every class and the head over the assembled U; then the merged walks, the
// one-workgroup kernel and the auxiliary stream of two-class plans.
static int setup_sectors(PlanBuild &b) {
    if (b.ss.cls.empty()) return GRAPE_OK;
    grape_plan *p = b.p;
    if (int rc = setup_sector_head(b)) return rc;
    grape_proj::SectorHead &H = p->SH;
    for (int cl = 0; cl < (int)b.ss.cls.size(); ++cl) {
        const SectorClass &sc = b.ss.cls[cl];
        if (dispatch_lds_limits(sc.S) != hipSuccess) return fail(GRAPE_ERR_HIP, "cannot raise LDS limit");
        std::vector<cd> sops((size_t)sc.nsec * b.n_ops * sc.S * sc.S), sopsT(sops.size());  // (rotated) operator blocks
        grape_setup::to_tiles(b.sdesc.ops, b.n_ops, p->P.D, sc.sidx.data(), sc.nsec, sc.S, sops.data(), sopsT.data());
        std::vector<int> gauge_n;
        decide_class(b, sc, sops, p->Ps[cl], gauge_n);
        if (int rc = alloc_class(b, cl, gauge_n, sops, sopsT)) return rc;
        // the lab-frame error walks' base table, once per plan
        if (p->Ps[cl].gauge_lab)
            if (int rc = fill_gauge_table(p, cl, true)) return rc;
        const grape_plan::SecBuf &sb = p->sb[cl];
        H.S[cl] = sc.S;
        H.nsec[cl] = sc.nsec;
        H.sidx[cl] = sb.sidx;
        H.Ub[cl] = sb.Ub;
        H.Msec[cl] = sb.Msec;
        H.TotS[cl] = sb.TotS;
        H.MsecE[cl] = sb.MsecE;
    }
    p->ncls = (int)b.ss.cls.size();
    if (int rc = setup_merge(b)) return rc;
    if (int rc = setup_eval1(p)) return rc;
    if (p->e1) p->wide = 0;  // (one workgroup per evaluation serves every call of such a plan)
    if (p->ncls == 2 && (hipStreamCreateWithFlags(&p->aux_stream, hipStreamNonBlocking) != hipSuccess ||
                         hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming) != hipSuccess ||
                         hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming) != hipSuccess))
        return fail(GRAPE_ERR_HIP, "cannot create the auxiliary stream");
    return GRAPE_OK;
}

// 12 < d <= 64 with GRAPE_OPT_GENERAL_H0, operator basis: the operator images and the problem
// ud_propagators_dev's dense branch exponentiates from (k_dexp<true> over the variant list): the terms,
// scalars and x layout are the general path's
static int setup_pivot_dense(PlanBuild &b) {
    if (!b.rt.pivot || b.rt.tables) return GRAPE_OK;
    grape_plan *p = b.p;
    const int D = p->P.D;
    if (grape_dense::set_lds_limits() != hipSuccess) return fail(GRAPE_ERR_HIP, "cannot raise LDS limit (dense)");
    const size_t IMG = grape_dense::kImgDoubles;
    std::vector<double> img((size_t)b.n_ops * IMG);
    for (int o = 0; o < b.n_ops; ++o) to_dense_image(b.desc->ops + 2 * (size_t)o * D * D, D, img.data() + o * IMG);
    if (p->mem.alloc(&p->dn_opimg, img.size()) != hipSuccess ||
        hipMemcpy(p->dn_opimg, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (dense operator images)");
    p->DP = grape_dense::DenseProblem{};
    p->DP.P = p->P;
    p->DP.opimg = p->dn_opimg;
    p->dense = true;
    return GRAPE_OK;
}

int create_small(PlanBuild &b) {
    if (int rc = setup_problem(b)) return rc;
    if (int rc = alloc_whole_matrix(b)) return rc;
    if (int rc = setup_general_h0(b)) return rc;
    if (int rc = setup_sectors(b)) return rc;
    return setup_pivot_dense(b);
}

}  // namespace grape_eng
