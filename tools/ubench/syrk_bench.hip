// syrk_bench.hip -- stand-alone correctness + timing harness for large_syrk_bf16x3 (P -= V V^T, ekf_large.h).
// Random V (binary32, n = 1027, columns n .. zero), P = 0: the kernel's P against a binary64 host product of the same V on sampled rows (the diagonal and
// the pose columns / rows are not the kernel's: large_x_update_rows forms those), exact symmetry, and the time of a launch -- for the two instantiations
// the library launches: <false> (per-slab temporaries, the default) and <true> (round 2's running accumulator, ASLAM_SYRK_RUNNING=1) -- and for <false>
// without the tail rule (ASLAM_SYRK_TAIL=0: the ninth tile row), whose P, padding included, must equal the default's bit for bit.
// The ablation variants behind the K-loop breakdown of profiles/r04_experiments.md section 2 are no longer in the kernel (profiles/README.md).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I awesomeslam_amd/csrc tools/ubench/syrk_bench.hip -o tools/ubench/syrk_bench && tools/ubench/syrk_bench [filters]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "ekf_large.h"

using namespace aslam;

#define CK(x)                                                                                                          \
        do                                                                                                             \
        {                                                                                                              \
                hipError_t e_ = (x);                                                                                   \
                if (e_ != hipSuccess)                                                                                  \
                {                                                                                                      \
                        std::printf("%s: %s\n", #x, hipGetErrorString(e_));                                            \
                        std::exit(1);                                                                                  \
                }                                                                                                      \
        } while (0)

template <typename F> float time_ms(F launch, int reps)
{
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0));
        CK(hipEventCreate(&e1));
        launch();
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0));
        for (int r = 0; r < reps; ++r)
                launch();
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        return ms / reps;
}

int main(int argc, char **argv)
{
        const int B = argc > 1 ? std::atoi(argv[1]) : 256;
        const int n = 1027, NP = 1088;
        const size_t M = (size_t)NP * NP;
        std::mt19937 rng(11);
        std::normal_distribution<float> nd;
        std::vector<float> V(M, 0.f);
        for (int i = 0; i <= n; ++i) // (row n = q rides along, as in the chain)
                for (int j = 0; j < n; ++j)
                        V[(size_t)i * NP + j] = nd(rng) * (1.0f + 0.01f * (float)(j % 7));
        float *dG;
        double *dP;
        int *dn, *dskip;
        CK(hipMalloc(&dG, sizeof(float) * M * B));
        CK(hipMalloc(&dP, sizeof(double) * M * B));
        CK(hipMalloc(&dn, sizeof(int) * B));
        CK(hipMalloc(&dskip, sizeof(int) * B));
        CK(hipMemset(dskip, 0, sizeof(int) * B));
        CK(hipMemset(dP, 0, sizeof(double) * M * B));
        for (int b = 0; b < B; ++b)
                CK(hipMemcpy(dG + M * b, V.data(), sizeof(float) * M, hipMemcpyHostToDevice));
        std::vector<int> nn(B, n);
        CK(hipMemcpy(dn, nn.data(), sizeof(int) * B, hipMemcpyHostToDevice));
        DevView d = {};
        d.B = B, d.NP = NP, d.n = dn;
        LargeView<float> lv = {};
        lv.NP = NP, lv.P = dP, lv.G = dG;
        lv.xrows = 1;
        lv.syrk_tail = 1; // (as the library launches <false>: n = 1027 = 8 x 128 + 3, the tail rows on the idle waves of the diagonal tiles; <true> keeps the ninth tile row)
        const int ntile = (NP + 127) / 128;
        const dim3 grid(8 * (ntile * (ntile + 1) / 2) * ((B + 7) / 8));
        const double sf = (ntile * (ntile + 1) / 2 - ntile * 0.25) * 2.0 * 128 * 128 * 1056 * B;
        std::vector<double> P(M), P0(M), Pprev;
        // ---- per instantiation: one launch on P = 0 -> P = -V V^T (lower + mirror), filters 0 and B - 1; then its time
        auto check_and_time = [&](const char *name, auto kern, bool same_as_previous) {
                CK(hipMemset(dP, 0, sizeof(double) * M * B));
                hipLaunchKernelGGL(kern, grid, dim3(256), 0, 0, d, lv, B, dskip);
                CK(hipDeviceSynchronize());
                CK(hipMemcpy(P0.data(), dP, sizeof(double) * M, hipMemcpyDeviceToHost));
                CK(hipMemcpy(P.data(), dP + M * (B - 1), sizeof(double) * M, hipMemcpyDeviceToHost));
                double worst = 0, asym = 0;
                size_t differ = 0;
                for (size_t i = 0; i < M; ++i)
                        differ += P[i] != P0[i];
                for (int i = 3; i < n; i += 13)
                        for (int j = 3; j < n; ++j)
                        {
                                if (i == j)
                                        continue;
                                double s = 0, sa = 0;
                                for (int k = 0; k < n; ++k)
                                {
                                        const double t = (double)V[(size_t)i * NP + k] * (double)V[(size_t)j * NP + k];
                                        s += t, sa += std::fabs(t);
                                }
                                worst = std::fmax(worst, std::fabs(-s - P[(size_t)i * NP + j]) / sa);
                                asym = std::fmax(asym, std::fabs(P[(size_t)i * NP + j] - P[(size_t)j * NP + i]));
                        }
                double untouched = 0;
                for (int i = 0; i < n; ++i)
                        untouched = std::fmax(untouched, std::fmax(std::fabs(P[(size_t)i * NP + i]), std::fmax(std::fabs(P[(size_t)i * NP + std::min(i, 2)]), std::fabs(P[(size_t)std::min(i, 2) * NP + i]))));
                double padding = 0;
                for (int i = 0; i < NP; ++i)
                        for (int j = (i < n ? n : 0); j < NP; ++j)
                                padding = std::fmax(padding, std::fabs(P[(size_t)i * NP + j]));
                std::printf("%s: max |P + V V^T| / sum |v v| = %.2e (rows 3, 16, ... of filter %d), asymmetry %.1e, entries of the pose columns / rows / diagonal written: %.1e, "
                            "padding past n written: %.1e, filter %d differs from filter 0 in %zu entries\n", name, worst, B - 1, asym, untouched, padding, B - 1, differ);
                if (same_as_previous)
                {
                        size_t d2 = 0;
                        for (size_t i = 0; i < M; ++i)
                                d2 += P[i] != Pprev[i];
                        std::printf("  P (all %d x %d entries) differs from the previous variant's in %zu entries\n", NP, NP, d2);
                }
                Pprev = P;
                const float ms = time_ms([&]() { hipLaunchKernelGGL(kern, grid, dim3(256), 0, 0, d, lv, B, dskip); }, 5);
                std::printf("  %-40s %8.3f ms for %d filters = %6.1f T fp32-equivalent FLOP/s executed\n", name, ms, B, sf / (ms * 1e-3) / 1e12);
        };
        check_and_time("syrk_bf16x3<false> (per-slab temporaries, tail rows on the diagonal tiles)", large_syrk_bf16x3<false>, false);
        lv.syrk_tail = 0;
        check_and_time("syrk_bf16x3<false> without the tail rule (ninth tile row)", large_syrk_bf16x3<false>, true);
        lv.syrk_tail = 1;
        check_and_time("syrk_bf16x3<true> (running accumulator)", large_syrk_bf16x3<true>, false);
        return 0;
}
