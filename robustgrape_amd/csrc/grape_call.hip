// grape_call.hip -- the call path of the C ABI: one call's launches on the plan's stream (enqueue*), the
// captured-graph path of small host-array calls, grape_fidelity_grad*, grape_plan_synchronize, the time
// slices, the host-table entry and per-kernel profiling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "grape_plan.hpp"

using namespace grape_eng;

namespace grape_eng {

// the dense engine's view of one launch (plan workspaces + the call's inputs and outputs)
static grape_dense::DenseBatch dense_batch(grape_plan *p, int nb, const double *d_x, double *d_F, double *d_Fdx,
                                           double *d_Fd2, double *d_Fd2dx) {
    grape_dense::DenseBatch DB{};
    DB.nb = nb;
    DB.x = d_x;
    DB.E = p->dn_E;
    DB.Q = p->dn_Q;
    DB.Carry = p->dn_Carry;
    DB.M = p->dn_M;
    DB.Mc = p->dn_Mc;
    DB.Z = p->dn_Z;
    DB.Ub = p->dn_Ub;
    DB.Zl = p->dn_Zl;
    DB.Vc = p->dn_Vc;
    DB.Sx = p->dn_Sx;
    DB.Tot = p->dn_Tot;
    DB.Me = p->dn_Me;
    DB.Mp = p->dn_Mp;
    DB.B0 = p->dn_B0;
    DB.Fd2 = d_Fd2;
    DB.Fd2dx = d_Fd2dx;
    DB.F = d_F;
    DB.Fdx = d_Fdx;
    DB.Fadd = p->dn_Fadd;
    DB.Fd2add = p->dn_Fd2add;
    DB.status = p->d_ctrl + 2;
    DB.mstats = nullptr;
    DB.gp_scr = p->d_gpscr;
    return DB;
}

grape_eval1::Args eval1_args(const grape_plan *p, const double *x, double *F, double *Fdx) {
    grape_eval1::Args A{};
    A.PA = p->Ps[p->e1_pa];
    A.PB = p->Ps[1 - p->e1_pa];
    A.H = p->SH;
    A.EtA = p->d_e1_Et;
    A.EtB = p->d_e1_Et + (size_t)A.PA.D * A.PA.D;
    A.x = x;
    A.F = F;
    A.Fdx = Fdx;
    A.a_first = p->e1_pa == 0 ? 1 : 0;
    A.trace = p->e1_trace_d;
    A.tab = p->d_e1_tab;
    return A;
}

// General H0 (p->general_h0): every evaluation of the launch through the materialised
// derivatives -- its propagator table, the chain and its LU inverses, the assembly
// (UnitaryCalculations.jl:44-155) -- then F, F_dx, F_d2err, F_d2err_dx from them
// (FidelityCalculations.jl:19-119), on the plan's stream, one evaluation after another in
// the single-evaluation workspace.
static int enqueue_general(grape_plan *p, int nb, const double *d_x, double *d_F, double *d_Fdx, double *d_Fd2,
                           double *d_Fd2dx, const KMark &mk) {
    if (int rc = ud_alloc(p)) return rc;
    const DevProblem &P = p->P;
    const size_t T = (size_t)P.D * P.D, nx = P.nx;
    hipStream_t st = p->stream;
    grape_unitary::UProblem UP;
    grape_unitary::UBuffers UB;
    const std::vector<grape::VSpec> vs = ud_setup(p, UP, UB);
    p->ud_vs_host = vs;  // the async copy reads this plan-owned copy
    HIPCHECK(hipMemcpyAsync(p->ud_vs, p->ud_vs_host.data(), vs.size() * sizeof(grape::VSpec), hipMemcpyHostToDevice, st));
    grape_unitary::FidArgs FA{};
    FA.P = P;
    FA.U = p->ud_C + (size_t)(P.Nt - 1) * T;
    FA.Udx = UB.Udx;
    FA.Udxa = UB.Udxa;
    FA.Ue = UB.Ue;
    FA.Uedx = UB.Uedx;
    FA.Uedxa = UB.Uedxa;
    FA.G = p->d_G;
    FA.scr = p->d_fscr;
    for (int b = 0; b < nb; ++b) {
        const double *xb = d_x + (size_t)b * nx;
        mk(GRAPE_KERNEL_EXPM, 0);
        if (int rc = ud_propagators_dev(p, xb, UP.nv,
                                        p->tables ? p->d_Htab + (size_t)b * P.Nt * UP.nv * T : nullptr)) return rc;
        mk(GRAPE_KERNEL_EXPM, 1);
        mk(GRAPE_KERNEL_GRAD, 0);
        HIPCHECK(grape_unitary::launch_assembly(UP, UB, st));
        FA.x = xb;
        FA.U0tab = p->tables ? p->d_U0tab + (size_t)b * (1 + P.na) * T : nullptr;
        FA.F = d_F + b;
        FA.Fdx = d_Fdx + (size_t)b * nx;
        FA.Fd2 = P.ne ? d_Fd2 + (size_t)b * P.ne : nullptr;
        FA.Fd2dx = P.ne ? d_Fd2dx + (size_t)b * P.ne * nx : nullptr;
        HIPCHECK(grape_unitary::launch_fidelity(FA, st));
        mk(GRAPE_KERNEL_GRAD, 1);
    }
    return GRAPE_OK;
}

// One launch sequence of `nb` evaluations on the plan's stream over workspace rows
// [0, nb).  The caller copies the status word afterwards.
static KMark profiling_mark(grape_plan *p) {  // per-kernel event pairs on the stream being enqueued (profiling on)
    KMark mk;
    if (p->profiling) {
        mk.ctx = p;
        mk.fn = [](void *ctx, int k, int phase) {
            grape_plan *pl = static_cast<grape_plan *>(ctx);
            hipEvent_t e = pl->get_event();
            if (!e) return;
            (void)hipEventRecord(e, pl->cur_stream);
            if (phase == 0) {
                pl->pending.push_back({k, e, nullptr});
            } else {
                pl->pending.back().b = e;
            }
        };
    }
    return mk;
}

// One wide pass (grape_walk_api.hpp launch_merged_wide) of nb == p->wide evaluations on the caller's buffers:
// the forward state walk, the head (k_wide_head: alpha per sector instead of the M blocks), the time-reversed
// gradient walk.  psi_N and the alphas live in the chunk totals' and the carries' buffers, which hold exactly
// max_batch x nchunks tiles per sector and are idle here (no chunks); later chunked passes follow in stream order.
// psi_N is evaluation-minor, entry j of chain ch of a class at [(ch * D + j) * nb + b] (twin sectors share chain 0).
static int enqueue_wide(grape_plan *p, int nb, const double *d_x, double *d_F, double *d_Fdx) {
    hipStream_t st = p->stream;
    p->cur_stream = st;
    const KMark mk = profiling_mark(p);
    const int ma = p->merge_pa, mb = 1 - ma;
    DevProblem Pw[2] = {p->Ps[ma], p->Ps[mb]};
    DevBatch Bw[2]{};
    for (int i = 0; i < 2; ++i) {
        const int cl = i == 0 ? ma : mb;
        const grape_plan::SecBuf &sb = p->sb[cl];
        Pw[i].nchunks = 1;
        Pw[i].L = Pw[i].Nt;
        Bw[i].nb = nb * Pw[i].nsec;
        Bw[i].x = d_x;
        Bw[i].F = d_F;
        Bw[i].Fdx = d_Fdx;
        Bw[i].Ub = sb.Tc;
        Bw[i].Msec = sb.Carry;
        Bw[i].status = p->d_ctrl + 2;
        Bw[i].sink = p->d_sink;
    }
    grape_proj::WideHead H{};
    H.P = p->SH.P;
    H.fixed = p->SH.fixed;
    H.nfixed = p->SH.nfixed;
    H.x = d_x;
    H.F = d_F;
    H.Fdx = d_Fdx;
    int ns = 0;
    for (int cl = 0; cl < 2; ++cl) {  // the sectors in the head's class order
        const DevProblem &Pc = p->Ps[cl];
        for (int w = 0; w < Pc.nsec; ++w, ++ns) {
            if (ns == 3) return fail(GRAPE_ERR_HIP, "wide pass: more than three sectors");
            const int ch = (cl == mb && Pc.twin) ? 0 : w;
            H.lev[ns] = p->wide_lev[cl][w];
            H.ucc[ns] = p->sb[cl].Tc + ((size_t)ch * Pc.D + Pc.rank1_c[w]) * nb;
            H.alpha[ns] = p->sb[cl].Carry + w;
            H.astride[ns] = Pc.nsec;
        }
    }
    if (ns != 3) return fail(GRAPE_ERR_HIP, "wide pass: fewer than three sectors");
    mk(GRAPE_KERNEL_WALK_FWD, 0);
    HIPCHECK(grape_walk::launch_merged_wide(0, Pw[0], Bw[0], Pw[1], Bw[1], st));
    mk(GRAPE_KERNEL_WALK_FWD, 1);
    mk(GRAPE_KERNEL_SCAN, 0);
    HIPCHECK(grape_proj::launch_wide_head(H, nb, st));
    mk(GRAPE_KERNEL_SCAN, 1);
    mk(GRAPE_KERNEL_WALK_GRAD, 0);
    HIPCHECK(grape_walk::launch_merged_wide(1, Pw[0], Bw[0], Pw[1], Bw[1], st));
    mk(GRAPE_KERNEL_WALK_GRAD, 1);
    return GRAPE_OK;
}

static int enqueue(grape_plan *p, int nb, const double *d_x, double *d_F, double *d_Fdx, double *d_Fd2,
                   double *d_Fd2dx) {
    hipStream_t st = p->stream;
    p->cur_stream = st;
    const KMark mk = profiling_mark(p);
    if (p->tiled) {  // one pass of nb <= max_batch evaluations in the plan's workspace (grape_tiled.hip)
        grape_tiled::TiledBatch TB = p->TB;
        TB.nb = nb;
        TB.x = d_x;
        TB.F = d_F;
        TB.Fdx = d_Fdx;
        TB.Fd2 = d_Fd2;  // (error sources, GRAPE_OPT_TILED_ERR: null otherwise)
        TB.Fd2dx = d_Fd2dx;
        HIPCHECK(grape_tiled::launch_pipeline(p->TP, TB, st, mk));
        return GRAPE_OK;
    }
    if (p->general_h0) return enqueue_general(p, nb, d_x, d_F, d_Fdx, d_Fd2, d_Fd2dx, mk);
    if (p->dense) {
        const grape_dense::DenseBatch DB = dense_batch(p, nb, d_x, d_F, d_Fdx, d_Fd2, d_Fd2dx);
        HIPCHECK(grape_dense::launch_pipeline(p->DP, DB, st, mk));
        return GRAPE_OK;
    }
    if (p->e1) {  // one workgroup per evaluation (grape_eval1.hip)
        mk(GRAPE_KERNEL_EVAL1, 0);
        HIPCHECK(grape_eval1::launch(eval1_args(p, d_x, d_F, d_Fdx), nb, st));
        mk(GRAPE_KERNEL_EVAL1, 1);
        return GRAPE_OK;
    }
    if (p->ncls) {  // sectors: stage 0 of every class, the head, stage 1 of every class, the sum
        DevBatch Bc[2]{};
        grape::SecParts sp{};
        for (int cl = 0; cl < p->ncls; ++cl) {
            const grape_plan::SecBuf &sb = p->sb[cl];
            DevBatch &B = Bc[cl];
            B.nb = nb * p->Ps[cl].nsec;
            B.x = d_x;
            B.F = d_F;
            B.Fdx = d_Fdx;
            B.E = sb.E;
            B.Q = sb.Q;
            B.Mc = sb.Mc;
            B.Carry = sb.Carry;
            B.Ub = sb.Ub;
            B.Msec = sb.Msec;
            B.part_add = p->d_part;
            B.tgt_part = p->d_tgt_part;
            B.overflow = sb.ovf;
            B.ovf2 = sb.ovf2;
            B.ovf2_slots = sb.slots;
            B.sec_part = sb.part;
            B.Fd2 = d_Fd2;
            B.Fd2dx = d_Fd2dx;
            B.part_err_add = p->d_part_err;
            if (p->P.ne > 0) {
                B.Zl = sb.Zl;
                B.Wc = p->Ps[cl].walk ? sb.Wc : nullptr;
                B.Me = sb.Me;
                B.TotS = sb.TotS;
                B.MsecE = sb.MsecE;
                B.sec_part_err = sb.part_err;
            }
            B.overflow_count = p->d_ctrl + 4 + 2 * cl;  // ctrl [4..7]: two counters per class
            B.ovf2_count = p->d_ctrl + 5 + 2 * cl;
            B.status = p->d_ctrl + 2;
            B.sink = p->d_sink;
            B.Tc = sb.Tc;  // chunk walks (null otherwise)
            B.wscr = sb.wscr;
            B.Ew = sb.Ew;
            sp.part[cl] = sb.part;
            sp.nsec[cl] = p->Ps[cl].walk ? grape_walk::grad_parts(p->Ps[cl]) : p->Ps[cl].nsec;
            if (p->merged && cl != p->merge_pa) sp.nsec[cl] = 0;  // (the merged walk's one part is class A's)
            sp.lane_major[cl] = p->Ps[cl].walk;  // k_walk_grad's / k_walk_img_sum's layout
            sp.part_err[cl] = sb.part_err;
            sp.lane_major_err[cl] = p->Ps[cl].walk;  // k_walk_err_grad's layout
        }
        bool parks = false;  // the chunk walks never park a step for k_expm_high: no counters to clear
        for (int cl = 0; cl < p->ncls; ++cl) parks = parks || !p->Ps[cl].walk;
        if (parks) HIPCHECK(hipMemsetAsync(p->d_ctrl + 4, 0, 4 * sizeof(int), st));
        // Small calls (latency-bound: the optimiser's line-search rounds, single evaluations) run
        // the second sector class on the auxiliary stream beside the first; large ones keep one
        // stream (no gain there, DESIGN 4.1, and per-kernel event times stay per kernel).
        const bool fork = p->aux_stream && !p->capturing && nb <= kForkMaxBatch &&
                          !(p->P.opts & GRAPE_OPT_NO_FORK);
        // Latency-bound calls of the Rydberg layout: both classes' walks (and scans) in ONE launch per
        // stage (grape_walk_api.hpp launch_pair) -- neither a graph branch nor a second stream overlaps
        // them inside a captured graph on this runtime.  pa: the 4- (or 3-) level class, pb: the 2-level one.
        int pa, pb;
        walk_pair_order(p, &pa, &pb);
        // (small calls only: a pair kernel runs the 2-level class at the 4-level class's occupancy)
        const bool pair = p->ncls == 2 && nb <= kPairMaxBatch && !(p->P.opts & GRAPE_OPT_NO_PAIR) &&
                          p->Ps[0].scan_waves == kScanLatency &&
                          p->Ps[1].scan_waves == kScanLatency && grape_walk::pair_ok(p->Ps[pa], p->Ps[pb]);
        auto stage = [&](int s) -> hipError_t {  // stage s of every class (class 1 forked when `fork`)
            if (p->merged && s < 2) {  // both classes in one lane (throughput passes)
                const int ma = p->merge_pa, mb = 1 - ma;
                mk(s == 0 ? GRAPE_KERNEL_WALK_FWD : GRAPE_KERNEL_WALK_GRAD, 0);
                hipError_t e = grape_walk::launch_merged(s, p->Ps[ma], Bc[ma], p->Ps[mb], Bc[mb], st);
                mk(s == 0 ? GRAPE_KERNEL_WALK_FWD : GRAPE_KERNEL_WALK_GRAD, 1);
                if (e == hipSuccess && s == 0) {  // the merged walks' sequential scan (lane-minor totals)
                    mk(GRAPE_KERNEL_SCAN, 0);
                    e = grape_walk::launch_merged(2, p->Ps[ma], Bc[ma], p->Ps[mb], Bc[mb], st);
                    mk(GRAPE_KERNEL_SCAN, 1);
                }
                return e;
            }
            if (pair && s < 2) {
                mk(s == 0 ? GRAPE_KERNEL_WALK_FWD : GRAPE_KERNEL_WALK_GRAD, 0);
                hipError_t e = grape_walk::launch_pair(s, p->Ps[pa], Bc[pa], p->Ps[pb], Bc[pb], st);
                mk(s == 0 ? GRAPE_KERNEL_WALK_FWD : GRAPE_KERNEL_WALK_GRAD, 1);
                if (e == hipSuccess && s == 0) {
                    mk(GRAPE_KERNEL_SCAN, 0);
                    e = p->Ps[pa].D == 4 ? grape_host::launch_scan_pair<4, 2>(p->Ps[pa], Bc[pa], p->Ps[pb], Bc[pb], st)
                                         : grape_host::launch_scan_pair<3, 2>(p->Ps[pa], Bc[pa], p->Ps[pb], Bc[pb], st);
                    mk(GRAPE_KERNEL_SCAN, 1);
                }
                return e;
            }
            if (s == 0 && !fork && !pair) {  // both walk classes' one-wave scans in one launch
                const int ca = p->Ps[0].D == 2 ? 1 : 0, cb = 1 - ca;
                const DevProblem &Pa = p->Ps[ca], &Pb = p->Ps[cb];
                if (p->ncls == 2 && Pa.walk && Pb.walk && (Pa.D == 3 || Pa.D == 4) && Pb.D == 2 &&
                    Pa.scan_waves == kScanTiny && Pb.scan_waves == kScanTiny) {
                    mk(GRAPE_KERNEL_WALK_FWD, 0);
                    hipError_t e = Pa.D == 4 ? grape_walk::launch<4>(0, Pa, Bc[ca], st) : grape_walk::launch<3>(0, Pa, Bc[ca], st);
                    if (e == hipSuccess) e = grape_walk::launch<2>(0, Pb, Bc[cb], st);
                    mk(GRAPE_KERNEL_WALK_FWD, 1);
                    if (e != hipSuccess) return e;
                    mk(GRAPE_KERNEL_SCAN, 0);
                    e = Pa.D == 4 ? grape_host::launch_scan_pair<4, 2, kScanTiny>(Pa, Bc[ca], Pb, Bc[cb], st)
                                  : grape_host::launch_scan_pair<3, 2, kScanTiny>(Pa, Bc[ca], Pb, Bc[cb], st);
                    mk(GRAPE_KERNEL_SCAN, 1);
                    return e;
                }
            }
            if (!fork || pair) {
                for (int cl = 0; cl < p->ncls; ++cl) {
                    const hipError_t e = dispatch_sector_stage(p->Ps[cl].D, s, p->Ps[cl], Bc[cl], p->FT, st, mk);
                    if (e != hipSuccess) return e;
                }
                return hipSuccess;
            }
            hipEvent_t evf = p->ev_fork, evj = p->ev_join;
            hipError_t e = hipEventRecord(evf, st);
            if (e == hipSuccess) e = hipStreamWaitEvent(p->aux_stream, evf, 0);
            if (e == hipSuccess) e = dispatch_sector_stage(p->Ps[0].D, s, p->Ps[0], Bc[0], p->FT, st, mk);
            p->cur_stream = p->aux_stream;
            if (e == hipSuccess) e = dispatch_sector_stage(p->Ps[1].D, s, p->Ps[1], Bc[1], p->FT, p->aux_stream, mk);
            p->cur_stream = st;
            if (e == hipSuccess) e = hipEventRecord(evj, p->aux_stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(st, evj, 0);
            return e;
        };
        HIPCHECK(stage(0));
        grape_proj::SectorHead H = p->SH;
        H.x = d_x;
        H.F = d_F;
        H.Fdx = d_Fdx;
        H.tgt_part = p->d_tgt_part;
        H.Fd2 = d_Fd2;
        H.Fd2dx = d_Fd2dx;
        mk(GRAPE_KERNEL_SCAN, 0);
        HIPCHECK(grape_proj::launch_sector_head(H, nb, st));
        mk(GRAPE_KERNEL_SCAN, 1);
        HIPCHECK(stage(1));
        if (p->P.ne > 0) {  // the sector error head, then the F_d2err_dx walks of every class
            mk(GRAPE_KERNEL_ERR_SCAN, 0);
            HIPCHECK(grape_proj::launch_sector_err_head(H, nb, st));
            mk(GRAPE_KERNEL_ERR_SCAN, 1);
            HIPCHECK(stage(2));
        }
        // (the merged gradient walk wrote F_dx itself; without x_add-dependent H0 nothing is left to sum)
        if (!(p->merged && !(p->P.xadd_dep && p->P.na > 0)))
            HIPCHECK(dispatch_sector_reduce(p->Ps[0].D, p->Ps[0], Bc[0], sp, nb, st, mk));
        return GRAPE_OK;
    }
    const DevProblem &P = p->P;
    DevBatch B{};
    B.Fd2 = d_Fd2;
    B.Fd2dx = d_Fd2dx;
    B.nb = nb;
    B.x = d_x;
    B.F = d_F;
    B.Fdx = d_Fdx;
    B.E = p->d_E;
    B.Q = p->d_Q;
    B.Mc = p->d_Mc;
    B.part_add = p->d_part;
    B.tgt_part = p->d_tgt_part;
    B.overflow = p->d_ovf;
    B.Carry = p->d_Carry;  // allocated for the error path and the general-projector heads
    B.Ub = p->d_Ub;
    B.gp_scr = p->d_gpscr;
    if (P.ne == 0) {
        B.ovf2 = p->d_ovf2;
        B.ovf2_slots = p->d_ovf2_slots;
    } else {
        B.Me = p->d_Me;
        B.part_err_add = p->d_part_err;
        B.Zl = p->d_Zl;
    }
    // ctrl: [2] status (sticky until grape_plan_synchronize reports it),
    // [4] k_expm overflow count, [5] k_expm_grad overflow count
    int *cnt = p->d_ctrl + 4;
    B.overflow_count = cnt;
    B.ovf2_count = cnt + 1;
    B.status = p->d_ctrl + 2;
    B.sink = p->d_sink;
    HIPCHECK(hipMemsetAsync(cnt, 0, 2 * sizeof(int), st));
    if (p->tables) {
        B.Htab = p->d_Htab;
        B.U0tab = p->d_U0tab;
    }
    HIPCHECK(dispatch_pipeline(P.D, P, B, p->FT, st, mk));
    return GRAPE_OK;
}

// Enqueue one call's batch, then copy the status word to pinned memory on the plan's stream.
// (Sector plans whose every class walks set no status bit -- no Pade solve, no parked step, no
// LU -- and skip that copy.)
static bool status_free(const grape_plan *p) {
    if (!p->ncls || p->general_h0 || p->dense || p->tables) return false;
    for (int cl = 0; cl < p->ncls; ++cl)
        if (!p->Ps[cl].walk) return false;
    return true;
}
static int enqueue_call(grape_plan *p, int nb, const double *d_x, double *d_F, double *d_Fdx, double *d_Fd2,
                        double *d_Fd2dx) {
    if (int rc = enqueue(p, nb, d_x, d_F, d_Fdx, d_Fd2, d_Fd2dx)) return rc;
    if (!status_free(p))
        HIPCHECK(hipMemcpyAsync(p->h_status, p->d_ctrl + 2, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    return GRAPE_OK;
}

static void resolve_events(grape_plan *p) {
    for (auto &pe : p->pending) {
        float ms = 0.f;
        if (pe.a && pe.b && hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess) {
            p->kernel_ms[pe.kernel] += ms;
            p->kernel_launches[pe.kernel] += 1;
        }
        if (pe.a) p->ev_pool.push_back(pe.a);
        if (pe.b) p->ev_pool.push_back(pe.b);
    }
    p->pending.clear();
}

}  // namespace grape_eng

extern "C" {

int grape_fidelity_grad_device_async(grape_plan *p, int nbatch, const double *d_x, double *d_F, double *d_F_dx,
                                     double *d_F_d2err, double *d_F_d2err_dx) {
    if (!p || nbatch < 0 || (nbatch > 0 && (!d_x || !d_F || !d_F_dx))) return fail(GRAPE_ERR_INVALID, "bad argument");
    if (p->tables) return fail(GRAPE_ERR_INVALID, "host-table plan: use grape_fidelity_grad_tables");
    if (p->P.ne > 0 && nbatch > 0 && (!d_F_d2err || !d_F_d2err_dx))
        return fail(GRAPE_ERR_INVALID, "error sources need F_d2err and F_d2err_dx outputs");
    HIPCHECK(hipSetDevice(p->device));
    // Device-resident batches of a rank-one merged plan: while at least W = max_batch x nchunks evaluations remain,
    // one wide pass of W (one lane per evaluation, no chunks: enqueue_wide); the rest through the chunked passes.
    // The path is chosen by count alone, so a repeated call repeats its bits.
    int b0 = 0;
    for (; p->wide > 0 && nbatch - b0 >= p->wide; b0 += p->wide)
        if (int rc = enqueue_wide(p, p->wide, d_x + (size_t)b0 * p->P.nx, d_F + b0, d_F_dx + (size_t)b0 * p->P.nx)) return rc;
    for (; b0 < nbatch; b0 += p->max_batch) {
        const int nb = std::min(p->max_batch, nbatch - b0);
        int rc = enqueue_call(p, nb, d_x + (size_t)b0 * p->P.nx, d_F + b0, d_F_dx + (size_t)b0 * p->P.nx,
                              p->P.ne ? d_F_d2err + (size_t)b0 * p->P.ne : nullptr,
                              p->P.ne ? d_F_d2err_dx + (size_t)b0 * p->P.ne * p->P.nx : nullptr);
        if (rc) return rc;
    }
    return GRAPE_OK;
}

int grape_plan_synchronize(grape_plan *p) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    HIPCHECK(hipSetDevice(p->device));
    HIPCHECK(hipStreamSynchronize(p->stream));
    resolve_events(p);
    const int st = *p->h_status;
    if (st & 3) {
        *p->h_status = 0;
        HIPCHECK(hipMemset(p->d_ctrl + 2, 0, sizeof(int)));
        return fail(GRAPE_ERR_SINGULAR, (st & 2) ? "singular propagator chain C_k (Julia inv would throw SingularException)"
                                                 : "singular Pade denominator (Julia gesv! would throw SingularException)");
    }
    return GRAPE_OK;
}

}  // extern "C"

namespace grape_eng {

// Host-array calls of at most kGraphBatch evaluations are latency-bound (a 1-evaluation C2
// call is ~10 dependent launches and copies of a few KB): they are captured once per batch size
// into a HIP graph -- pinned staging copies in, the pipeline, status and results out -- and
// replayed with one launch.  GRAPE_NO_GRAPH=1 (or profiling) takes the stream path.
constexpr int kGraphBatch = 64, kGraphCache = 8;

// offsets (doubles) of the outputs of a graph-path call of nb evaluations in p->d_gout / p->h_F:
// F [B], F_dx [nb][nx], F_d2err [nb][ne], F_d2err_dx [nb][ne][nx] (B = the graph path's batch capacity);
// used = the extent one D2H copy returns
struct GraphOut {
    size_t fdx, fd2, fd2dx, used, capacity;
};
static GraphOut graph_out(const grape_plan *p, int nb) {
    const size_t nx = p->P.nx, ne = p->P.ne, B = std::min(kGraphBatch, p->max_batch);
    GraphOut o;
    o.fdx = B;
    o.fd2 = B * (1 + nx);
    o.fd2dx = o.fd2 + B * ne;
    o.used = ne ? o.fd2dx + (size_t)nb * ne * nx : o.fdx + (size_t)nb * nx;
    o.capacity = o.fd2dx + B * ne * nx;
    return o;
}

static int graph_capture(grape_plan *p, int nb, hipGraphExec_t *out) {
    const int nx = p->P.nx, ne = p->P.ne;
    hipStream_t st = p->stream;
    HIPCHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    auto body = [&]() -> int {
        HIPCHECK(hipMemcpyAsync(p->d_x, p->h_x, (size_t)nb * nx * sizeof(double), hipMemcpyHostToDevice, st));
        // every output in one device block [F | F_dx | F_d2err | F_d2err_dx] (graph_out), returned by ONE
        // D2H copy into its pinned image (round 6: one copy instead of three with error sources, ~9 us
        // of a 0.09-ms single evaluation)
        const GraphOut o = graph_out(p, nb);
        if (int rc = enqueue_call(p, nb, p->d_x, p->d_gout, p->d_gout + o.fdx, p->d_gout + o.fd2, p->d_gout + o.fd2dx))
            return rc;
        HIPCHECK(hipMemcpyAsync(p->h_F, p->d_gout, o.used * sizeof(double), hipMemcpyDeviceToHost, st));
        return GRAPE_OK;
    };
    p->capturing = true;
    const int rc = body();
    p->capturing = false;
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &g);
    if (rc) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess) return fail(GRAPE_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(e));
    hipGraphExec_t ex = nullptr;
    const hipError_t ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) return fail(GRAPE_ERR_HIP, std::string("graph instantiate: ") + hipGetErrorString(ei));
    if ((int)p->graphs.size() >= kGraphCache) {
        (void)hipGraphExecDestroy(p->graphs.front().exec);
        p->graphs.erase(p->graphs.begin());
    }
    p->graphs.push_back({nb, ex});
    *out = ex;
    return GRAPE_OK;
}

static bool graph_path(const grape_plan *p, int nbatch) {
    const bool disabled = (p->P.opts & GRAPE_OPT_NO_GRAPH) != 0;
    return !disabled && !p->profiling && !p->tables && !p->general_h0 && !p->tiled && nbatch > 0 && nbatch <= kGraphBatch &&
           nbatch <= p->max_batch;
}

static int fidelity_grad_graph(grape_plan *p, int nb, const double *x, double *F, double *F_dx, double *F_d2err,
                               double *F_d2err_dx) {
    const size_t nx = p->P.nx, ne = p->P.ne, B = std::min(kGraphBatch, p->max_batch);
    if (!p->h_x) {
        auto pin = [](double **h, size_t n) {
            return hipHostMalloc(reinterpret_cast<void **>(h), std::max<size_t>(n, 1) * sizeof(double),
                                 hipHostMallocDefault) == hipSuccess;
        };
        const size_t cap = graph_out(p, 1).capacity;
        if (!pin(&p->h_x, B * nx) || !pin(&p->h_F, cap))
            return fail(GRAPE_ERR_ALLOC, "pinned allocation failed (graph path)");
        if (p->mem.alloc(&p->d_gout, cap) != hipSuccess)
            return fail(GRAPE_ERR_ALLOC, "device allocation failed (graph path)");
    }
    if (p->e1) {
        // one workgroup per evaluation: a single launch that reads x from and writes F, F_dx to the
        // mapped pinned buffers -- no staging copies, no graph
        if (!p->hd_x && (hipHostGetDevicePointer(reinterpret_cast<void **>(&p->hd_x), p->h_x, 0) != hipSuccess ||
                         hipHostGetDevicePointer(reinterpret_cast<void **>(&p->hd_F), p->h_F, 0) != hipSuccess))
            return fail(GRAPE_ERR_HIP, "pinned buffers are not mapped (eval1)");
        std::memcpy(p->h_x, x, (size_t)nb * nx * sizeof(double));
        if (int rc = enqueue_call(p, nb, p->hd_x, p->hd_F, p->hd_F + B, nullptr, nullptr)) return rc;
        if (int rc = grape_plan_synchronize(p)) return rc;
        std::memcpy(F, p->h_F, (size_t)nb * sizeof(double));
        std::memcpy(F_dx, p->h_F + B, (size_t)nb * nx * sizeof(double));
        if (p->e1_trace) {
            const long long *tr = p->e1_trace;
            for (int i = 0; i < 9; ++i) p->e1_phase[i] += (double)(tr[i + 1] - tr[i]);
            const double us = (double)(tr[15] - tr[14]) / 100.0;  // (wall clock: 100 MHz)
            if (us > 0) p->e1_phase[9] += (double)(tr[9] - tr[0]) / us;
            for (int i = 0; i < 4; ++i) p->e1_phase[10 + i] += (double)(tr[17 + i] - tr[16 + i]);
            p->e1_phase[14] += (double)(tr[21] - tr[1]);
            p->e1_phase[15] += (double)(tr[22] - tr[1]);
            p->e1_calls += 1;
        }
        return GRAPE_OK;
    }
    hipGraphExec_t ex = nullptr;
    for (auto &g : p->graphs)
        if (g.nb == nb) ex = g.exec;
    if (!ex)
        if (int rc = graph_capture(p, nb, &ex)) return rc;
    std::memcpy(p->h_x, x, (size_t)nb * nx * sizeof(double));
    HIPCHECK(hipGraphLaunch(ex, p->stream));
    if (int rc = grape_plan_synchronize(p)) return rc;
    const GraphOut o = graph_out(p, nb);
    std::memcpy(F, p->h_F, (size_t)nb * sizeof(double));
    std::memcpy(F_dx, p->h_F + o.fdx, (size_t)nb * nx * sizeof(double));
    if (ne > 0) {
        std::memcpy(F_d2err, p->h_F + o.fd2, (size_t)nb * ne * sizeof(double));
        std::memcpy(F_d2err_dx, p->h_F + o.fd2dx, (size_t)nb * ne * nx * sizeof(double));
    }
    return GRAPE_OK;
}

// the results of workspace rows [0, nb) into the caller's host arrays at evaluation b0; synchronises
static int results_to_host(grape_plan *p, int b0, int nb, double *F, double *F_dx, double *F_d2err, double *F_d2err_dx) {
    const size_t nx = p->P.nx, ne = p->P.ne;
    HIPCHECK(hipMemcpyAsync(F + b0, p->d_F, nb * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    if (ne > 0) {
        HIPCHECK(hipMemcpyAsync(F_d2err + b0 * ne, p->d_Fd2, nb * ne * sizeof(double), hipMemcpyDeviceToHost, p->stream));
        HIPCHECK(hipMemcpyAsync(F_d2err_dx + b0 * ne * nx, p->d_Fd2dx, nb * ne * nx * sizeof(double),
                                hipMemcpyDeviceToHost, p->stream));
    }
    HIPCHECK(hipMemcpyAsync(F_dx + b0 * nx, p->d_Fdx, nb * nx * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    return grape_plan_synchronize(p);
}

}  // namespace grape_eng

extern "C" {

int grape_fidelity_grad(grape_plan *p, int nbatch, const double *x, double *F, double *F_dx, double *F_d2err,
                        double *F_d2err_dx) {
    if (!p || nbatch < 0 || (nbatch > 0 && (!x || !F || !F_dx))) return fail(GRAPE_ERR_INVALID, "bad argument");
    if (p->tables) return fail(GRAPE_ERR_INVALID, "host-table plan: use grape_fidelity_grad_tables");
    if (p->P.ne > 0 && nbatch > 0 && (!F_d2err || !F_d2err_dx))
        return fail(GRAPE_ERR_INVALID, "error sources need F_d2err and F_d2err_dx outputs");
    HIPCHECK(hipSetDevice(p->device));
    if (graph_path(p, nbatch)) return fidelity_grad_graph(p, nbatch, x, F, F_dx, F_d2err, F_d2err_dx);
    const int nx = p->P.nx;
    for (int b0 = 0; b0 < nbatch; b0 += p->max_batch) {
        const int nb = std::min(p->max_batch, nbatch - b0);
        HIPCHECK(hipMemcpyAsync(p->d_x, x + (size_t)b0 * nx, (size_t)nb * nx * sizeof(double),
                                hipMemcpyHostToDevice, p->stream));
        if (int rc = enqueue_call(p, nb, p->d_x, p->d_F, p->d_Fdx, p->d_Fd2, p->d_Fd2dx)) return rc;
        if (int rc = results_to_host(p, b0, nb, F, F_dx, F_d2err, F_d2err_dx)) return rc;
    }
    return GRAPE_OK;
}

}  // extern "C"

namespace grape_eng {

// Time sharding of one evaluation: see include/grape.h.
static int slice_check(grape_plan *p) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    if (p->tiled) return fail(GRAPE_ERR_UNSUPPORTED, "time slices: not served by the tiled engine (ndim > GRAPE_MAX_DENSE_DIM)");
    if (!p->dense || p->general_h0 || p->tables || p->P.ne > 0 || p->P.na > 0 || p->P.gen_proj || p->uses_tstep)
        return fail(GRAPE_ERR_UNSUPPORTED, "time slices: dense-engine operator-basis plans without error sources, "
                                           "x_add, a general projector or step-index terms");
    const size_t T = (size_t)p->P.D * p->P.D;
    if (!p->dn_Ub && p->mem.alloc(&p->dn_Ub, (size_t)p->max_batch * grape_dense::kImgDoubles) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (time slices)");
    if (!p->d_slice && p->mem.alloc(&p->d_slice, 2 * T) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (time slices)");
    return GRAPE_OK;
}

}  // namespace grape_eng

extern "C" {

int grape_slice_forward(grape_plan *p, const double *x, double *U_slice) {
    if (!p || !x || !U_slice) return fail(GRAPE_ERR_INVALID, "bad argument");
    HIPCHECK(hipSetDevice(p->device));
    if (int rc = slice_check(p)) return rc;
    const size_t T = (size_t)p->P.D * p->P.D;
    hipStream_t st = p->stream;
    HIPCHECK(hipMemcpyAsync(p->d_x, x, (size_t)p->P.nx * sizeof(double), hipMemcpyHostToDevice, st));
    const grape_dense::DenseBatch DB = dense_batch(p, 1, p->d_x, p->d_F, p->d_Fdx, nullptr, nullptr);
    HIPCHECK(grape_dense::launch_slice_forward(p->DP, DB, p->d_slice, st));
    HIPCHECK(hipMemcpyAsync(p->h_status, p->d_ctrl + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(U_slice, p->d_slice, T * sizeof(cd), hipMemcpyDeviceToHost, st));
    return grape_plan_synchronize(p);
}

int grape_slice_gradient(grape_plan *p, const double *M_prime, double *F_dx) {
    if (!p || !M_prime || !F_dx) return fail(GRAPE_ERR_INVALID, "bad argument");
    HIPCHECK(hipSetDevice(p->device));
    if (int rc = slice_check(p)) return rc;
    const size_t T = (size_t)p->P.D * p->P.D;
    hipStream_t st = p->stream;
    HIPCHECK(hipMemcpyAsync(p->d_slice + T, M_prime, T * sizeof(cd), hipMemcpyHostToDevice, st));
    const grape_dense::DenseBatch DB = dense_batch(p, 1, p->d_x, p->d_F, p->d_Fdx, nullptr, nullptr);
    HIPCHECK(grape_dense::launch_slice_gradient(p->DP, DB, p->d_slice + T, st));
    HIPCHECK(hipMemcpyAsync(p->h_status, p->d_ctrl + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(F_dx, p->d_Fdx, (size_t)p->P.np * p->P.Nt * sizeof(double), hipMemcpyDeviceToHost, st));
    return grape_plan_synchronize(p);
}

int grape_slice_forward_device(grape_plan *p, const double *d_x, double *d_U_slice) {
    if (!p || !d_x || !d_U_slice) return fail(GRAPE_ERR_INVALID, "bad argument");
    HIPCHECK(hipSetDevice(p->device));
    if (int rc = slice_check(p)) return rc;
    hipStream_t st = p->stream;
    // the slice's controls stay in the plan for grape_slice_gradient_device (as the host entry)
    HIPCHECK(hipMemcpyAsync(p->d_x, d_x, (size_t)p->P.nx * sizeof(double), hipMemcpyDeviceToDevice, st));
    const grape_dense::DenseBatch DB = dense_batch(p, 1, p->d_x, p->d_F, p->d_Fdx, nullptr, nullptr);
    HIPCHECK(grape_dense::launch_slice_forward(p->DP, DB, reinterpret_cast<cd *>(d_U_slice), st));
    // the Pade status for the caller's grape_plan_synchronize (as the host entries report it)
    HIPCHECK(hipMemcpyAsync(p->h_status, p->d_ctrl + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    return GRAPE_OK;
}

int grape_slice_gradient_device(grape_plan *p, const double *d_M_prime, double *d_F_dx) {
    if (!p || !d_M_prime || !d_F_dx) return fail(GRAPE_ERR_INVALID, "bad argument");
    HIPCHECK(hipSetDevice(p->device));
    if (int rc = slice_check(p)) return rc;
    const grape_dense::DenseBatch DB = dense_batch(p, 1, p->d_x, p->d_F, d_F_dx, nullptr, nullptr);
    HIPCHECK(grape_dense::launch_slice_gradient(p->DP, DB, reinterpret_cast<const cd *>(d_M_prime), p->stream));
    HIPCHECK(hipMemcpyAsync(p->h_status, p->d_ctrl + 2, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    return GRAPE_OK;
}

int grape_fidelity_grad_tables(grape_plan *p, int nbatch, const double *x, const double *H, const double *U0,
                               double *F, double *F_dx, double *F_d2err, double *F_d2err_dx) {
    if (!p || nbatch < 0 || (nbatch > 0 && (!x || !H || !U0 || !F || !F_dx)))
        return fail(GRAPE_ERR_INVALID, "bad argument");
    if (p && p->P.ne > 0 && nbatch > 0 && (!F_d2err || !F_d2err_dx))
        return fail(GRAPE_ERR_INVALID, "error sources need F_d2err and F_d2err_dx outputs");
    if (!p->tables) return fail(GRAPE_ERR_INVALID, "plan was not created with GRAPE_DESC_HOST_TABLES");
    HIPCHECK(hipSetDevice(p->device));
    const DevProblem &P = p->P;
    const size_t nx = P.nx, T = (size_t)P.D * P.D, hsz = (size_t)P.Nt * P.nv * T, usz = (1 + (size_t)P.na) * T;
    for (int b0 = 0; b0 < nbatch; b0 += p->max_batch) {
        const int nb = std::min(p->max_batch, nbatch - b0);
        HIPCHECK(hipMemcpyAsync(p->d_x, x + b0 * nx, nb * nx * sizeof(double), hipMemcpyHostToDevice, p->stream));
        HIPCHECK(hipMemcpyAsync(p->d_Htab, H + 2 * b0 * hsz, nb * hsz * sizeof(cd), hipMemcpyHostToDevice,
                                p->stream));
        HIPCHECK(hipMemcpyAsync(p->d_U0tab, U0 + 2 * b0 * usz, nb * usz * sizeof(cd), hipMemcpyHostToDevice,
                                p->stream));
        if (int rc = enqueue_call(p, nb, p->d_x, p->d_F, p->d_Fdx, p->d_Fd2, p->d_Fd2dx)) return rc;
        if (int rc = results_to_host(p, b0, nb, F, F_dx, F_d2err, F_d2err_dx)) return rc;
    }
    return GRAPE_OK;
}

int grape_plan_set_profiling(grape_plan *p, int enable) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    p->profiling = enable != 0;
    return GRAPE_OK;
}

int grape_plan_kernel_times(grape_plan *p, double *total_ms, long long *launches, int reset) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    for (int k = 0; k < GRAPE_NUM_KERNELS; ++k) {
        if (total_ms) total_ms[k] = p->kernel_ms[k];
        if (launches) launches[k] = p->kernel_launches[k];
        if (reset) {
            p->kernel_ms[k] = 0.0;
            p->kernel_launches[k] = 0;
        }
    }
    return GRAPE_OK;
}

}  // extern "C"
