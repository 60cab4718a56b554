// The tiled engine's product kernel on its own (grape_tiled.hpp tile_product): C_i = A_i B_i over n items of
// P x P complex FP64 images, timed with HIP events after a warm-up, credited 8 P^3 FLOP per product, and
// checked on a few entries of a few items against a host sum.  Build and run (from the repository root):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Iinclude -Irobustgrape_amd/csrc \
//       scripts/probes/tiled_product_probe.hip -o scripts/probes/tiled_product_probe
//   scripts/probes/tiled_product_probe [d = 128] [items = 1024] [reps = 20]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "grape_tiled.hpp"

using namespace grape_tiled;

template <bool LCT, bool RCT>
__global__ __launch_bounds__(NTHREADS) void k_probe(Geo g, const double *A, const double *B, double *C) {
    __shared__ double lds[4 * SLAB];
    const size_t img = 2 * (size_t)g.P * g.P, off = (size_t)(blockIdx.x >> 2) * img;
    Ops o;
    o.L = A + off;
    o.R = B + off;
    o.C = C + off;
    tile_product<LCT, RCT>(g, o, (int)(blockIdx.x & 3), lds);
}

// entries in [-1, 1) from a hash of the index; the padding (rows / columns >= d) stays zero
__global__ void k_fill(double *X, size_t n, int P, int d, unsigned seed) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t e = i % ((size_t)P * P);
    const int row = (int)(e / P), col = (int)(e % P);
    unsigned h = (unsigned)(i * 2654435761u) ^ seed;
    h ^= h >> 15;
    h *= 2246822519u;
    h ^= h >> 13;
    X[i] = (row < d && col < d) ? (double)(h & 0xffffff) / 8388608.0 - 1.0 : 0.0;
}

#define CHECK(x)                                                                  \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));          \
            return 2;                                                             \
        }                                                                         \
    } while (0)

template <bool LCT, bool RCT>
static int run(const char *name, Geo g, const double *A, const double *B, double *C, int n, int reps) {
    const int P = g.P;
    const size_t plane = (size_t)P * P, img = 2 * plane;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int r = 0; r < 3; ++r) hipLaunchKernelGGL((k_probe<LCT, RCT>), dim3(n * 4u), dim3(NTHREADS), 0, 0, g, A, B, C);
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(e0, 0));
    for (int r = 0; r < reps; ++r) hipLaunchKernelGGL((k_probe<LCT, RCT>), dim3(n * 4u), dim3(NTHREADS), 0, 0, g, A, B, C);
    CHECK(hipEventRecord(e1, 0));
    CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    // a few entries of the first and the last item against a host sum
    double worst = 0.0;
    for (int item : {0, n - 1}) {
        std::vector<double> a(img), b(img), c(img);
        CHECK(hipMemcpy(a.data(), A + (size_t)item * img, img * 8, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(b.data(), B + (size_t)item * img, img * 8, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(c.data(), C + (size_t)item * img, img * 8, hipMemcpyDeviceToHost));
        auto el = [&](const std::vector<double> &m, bool ct, int i, int j, double &re, double &im) {
            const size_t o = ct ? (size_t)j * P + i : (size_t)i * P + j;
            re = m[o];
            im = ct ? -m[plane + o] : m[plane + o];
        };
        for (int i : {0, 17, 63, 64, P - 1})
            for (int j : {0, 5, 64, P - 16, P - 1}) {
                double sr = 0.0, si = 0.0;
                for (int k = 0; k < P; ++k) {
                    double ar, ai, br, bi;
                    el(a, LCT, i, k, ar, ai);
                    el(b, RCT, k, j, br, bi);
                    sr += ar * br - ai * bi;
                    si += ar * bi + ai * br;
                }
                worst = std::fmax(worst, std::fmax(std::fabs(sr - c[(size_t)i * P + j]), std::fabs(si - c[plane + (size_t)i * P + j])));
            }
    }
    const double per = ms / reps, flop = 8.0 * P * P * P * n;
    std::printf("{\"probe\": \"tiled_product\", \"form\": \"%s\", \"d\": %d, \"P\": %d, \"items\": %d, \"reps\": %d, "
                "\"ms_per_launch\": %.4f, \"tflops_credited_8P3\": %.3f, \"frac_of_78.6\": %.4f, \"max_abs_err\": %.3e}\n",
                name, g.d, P, n, reps, per, flop / (per * 1e-3) / 1e12, flop / (per * 1e-3) / 1e12 / 78.6, worst);
    return worst < 1e-11 ? 0 : 1;
}

int main(int argc, char **argv) {
    const int d = argc > 1 ? std::atoi(argv[1]) : 128, n = argc > 2 ? std::atoi(argv[2]) : 1024,
              reps = argc > 3 ? std::atoi(argv[3]) : 20;
    if (d <= 64 || d > 128 || n < 1 || reps < 1) {
        std::fprintf(stderr, "usage: tiled_product_probe [64 < d <= 128] [items] [reps]\n");
        return 2;
    }
    const int P = 16 * ((d + 15) / 16);
    const Geo g{P, d};
    const size_t total = 2 * (size_t)P * P * n;
    double *A, *B, *C;
    CHECK(hipMalloc(&A, total * 8));
    CHECK(hipMalloc(&B, total * 8));
    CHECK(hipMalloc(&C, total * 8));
    const unsigned blocks = (unsigned)((total + 255) / 256);
    hipLaunchKernelGGL(k_fill, dim3(blocks), dim3(256), 0, 0, A, total, P, d, 1u);
    hipLaunchKernelGGL(k_fill, dim3(blocks), dim3(256), 0, 0, B, total, P, d, 2u);
    CHECK(hipDeviceSynchronize());
    int rc = run<false, false>("L R", g, A, B, C, n, reps);
    rc |= run<true, false>("L^dag R", g, A, B, C, n, reps);
    rc |= run<false, true>("L R^dag", g, A, B, C, n, reps);
    (void)hipFree(A);
    (void)hipFree(B);
    (void)hipFree(C);
    return rc;
}
