// grape_tiled_api.hpp -- what the C ABI (grape_engine.hip) sees of the tiled
// engine (grape_tiled.hip, GRAPE_MAX_DENSE_DIM < d <= GRAPE_MAX_TILED_DIM): the
// problem / batch descriptors, the workspace layout and the launchers.
#pragma once
#include <hip/hip_runtime.h>

#include "grape_launch_api.hpp"

namespace grape_tiled {

// d padded to the MFMA tile: 80, 96, 112 or 128 for 64 < d <= 128
inline int padded_dim(int d) { return 16 * ((d + 15) / 16); }
// doubles of one image: re plane then im plane, row-major Pd x Pd, zero padding
inline size_t image_doubles(int d) { return 2 * (size_t)padded_dim(d) * padded_dim(d); }

// (kMaxTerms, the H0 / target terms a tiled plan serves: grape_types.hpp)

// Scalars and term tables are shared with the other engines (DevProblem: ops / opsT / vs unused
// here); the operator basis is stored as images.
struct TiledProblem {
    grape::DevProblem P;
    int Pd;               // padded dimension
    const double *opimg;  // [n_ops][image]
    const double *W;      // [Pd] projector diagonal, zero-padded
    int Lc, Nc;           // chunk length / count of the prefix products
};

// Workspace of the exponential: one slab of `slab` items (images each)
struct ExpSlab {
    int slab;
    double *A, *A2, *A3, *A4, *B0, *B1;  // A / 2^s and its powers, the two Horner / squaring buffers
};

struct TiledBatch {
    int nb;
    const double *x;  // [nb][nx]
    double *E;        // [nb][Nt]       nominal propagators
    double *Q;        // [nb][Nt]       chunk-local prefix products (a chunk's first step lives in E)
    double *Carry;    // [nb][Nc]       C at the chunk starts, c >= 2 (c = 1 is a prefix, c = 0 the identity)
    double *Tm;       // [nb][Nc]       Carry_c M
    double *Mc;       // [nb][Nc]       Carry_c M Carry_c^dagger, c >= 1 (c = 0 is M)
    double *U, *M, *WK, *T;  // [nb] each: U = C_Nt, M = G U, W K, K^dag W K
    double *U0;       // [nb][1 + na]   target, then its eps-differences in x_add
    double *K;        // [nb][1 + na]   U0^dag U, dU0_q^dag U
    double *tau;      // [nb][2]
    ExpSlab X;
    double *Ev;       // [slab]         eps-variant propagators of the current slab (never kept)
    double *Ts, *Yd;  // [slab]         Q_{k-1} M'_c and Y_k^dagger of the current slab
    int *ctl;         // [nb][Nt]       Taylor block count and squaring count of every step
    int *smax;        // device word: the largest squaring count of the pass
    int *h_smax;      // ... its pinned copy (one word read back per pass)
    double *F;        // [nb]
    double *Fdx;      // [nb][nx]
    // error sources (P.ne > 0, GRAPE_OPT_TILED_ERR; null otherwise).  Local-frame images are kept conjugate-
    // transposed (Zd = Z^dag), so that every trace against them is an elementwise sum and W enters the
    // products through op()
    double *Zl;       // [nb][Nt][nz]   Z1_u^dag (np) | W_e^dag (ne) | Z2_{e,u}^dag (ne x np), nz = np + ne + ne np
    double *Sd, *Tmp; // [nb][ne][Nc]   (sum of W over the chunk)^dag, c >= 1; the first product of a pair
    double *Vc, *Sx, *Dx;     // [nb][ne][Nc]  Carry^dag (sum W) Carry, its exclusive prefix S_c, Tot - S_c
    double *Mce, *Tce, *Dce;  // [nb][ne][Nc]  Carry (M_e | S_c | Tot - S_c) Carry^dag, c >= 1 (c = 0: the images themselves)
    double *Bst, *Lam;        // [nb][ne][Nc]  the walk's state B_k and -Lambda_k
    double *Tot, *Ue, *UeU, *KW, *Me;  // [nb][ne] each: Tot, U Tot, Ue^dag U, Ke^dag W K, M_e = G_e U
    double *Ke;       // [nb][ne][1 + na]  U0^dag Ue, dU0_q^dag Ue
    double *taue;     // [nb][ne][2]       tau_e = tr(W Ke)
    double *Eh;       // [np + 1][slab]   held eps2-variants of the current slab: x + eps2 e_u (np), then source e
    double *Fd2;      // [nb][ne]
    double *Fd2dx;    // [nb][ne][nx]
};

// images per evaluation / per slab item that the error path adds to a plan's workspace (grape_plan_build.hip)
inline size_t err_eval_images(size_t Nt, size_t Nc, size_t np, size_t na, size_t ne) {
    return ne ? Nt * (np + ne + ne * np) + ne * (10 * Nc + 5 + 1 + na) : 0;
}
inline size_t err_slab_images(size_t np, size_t ne) { return ne ? np + 1 : 0; }

// Pipeline of one pass on `st` (the dense engine's stages and timing slots).  Reads one word back
// (the pass's largest squaring count) after the step norms: the call synchronises `st` once.
hipError_t launch_pipeline(const TiledProblem &P, const TiledBatch &B, hipStream_t st, const grape_host::KMark &mark);

// n exponentials of images (grape_expm_batch for 64 < d <= 128, skew-Hermitian or any A of moderate norm:
// Taylor by Paterson-Stockmeyer in A^4 after scaling to |A / 2^s|_1 <= 0.95, then s squarings).
// ctl [n], smax and mstats [5] device words (zeroed by the caller); h_smax pinned.  Synchronises `st`.
hipError_t launch_expm_raw(int d, const double *A, double *E, int n, const ExpSlab &X, int *ctl, int *smax,
                           int *h_smax, int *mstats, hipStream_t st);

}  // namespace grape_tiled
