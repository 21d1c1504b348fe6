// Micro-benchmark + accuracy check of the split-bf16 fp32 GEMM (g-meta_amd/csrc/gemm_split.h: the persistent three-piece kernel the library ships,
// 128 x 256 tiles) against an fp64 reference and the plain fp32 fmaf chain, at the arxiv query-layer shape (rows x 256 x 256).
//   hipcc --offload-arch=gfx950 -O3 -o tools/_build/gemm_split_bench tools/gemm_split_bench.hip && tools/_build/gemm_split_bench [M [K [N]]]
// Environment: GS_HALF=1 64-row half tiles (two workgroups per tile), GS_GRID=n grid cap (default 256), GS_NT=0 ordinary C stores,
// GS_SLEEP_US=n "cool chip" mode.  Exit status 0 if the error against fp64 is within 20x the fmaf chain's, else 2.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include <algorithm>
#include <unistd.h>
#include "../g-meta_amd/csrc/gemm_split.h"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s failed: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

int main(int argc, char** argv) {
    const int M = argc > 1 ? atoi(argv[1]) : 1146880, K = argc > 2 ? atoi(argv[2]) : 256, N = argc > 3 ? atoi(argv[3]) : 256;
    if (M <= 0 || K < 32 || K % 16 || N != 256) { printf("usage: gemm_split_bench [M [K [N]]]   K a multiple of 16, at least 32; N = 256 (the 256-wide tiles)\n"); return 1; }
    const bool half = getenv("GS_HALF") != nullptr;
    const int cap = getenv("GS_GRID") ? atoi(getenv("GS_GRID")) : 256;
    printf("M=%d K=%d N=%d %s tiles, grid cap %d\n", M, K, N, half ? "half" : "full", cap);
    std::vector<float> A((size_t)M * K), W((size_t)K * N), bias(N);
    srand(1);
    auto rnd = []() { return (float)((rand() / (double)RAND_MAX) * 2.0 - 1.0); };
    for (auto& v : W) v = rnd() * 0.1f;
    for (auto& v : bias) v = rnd();
    for (size_t i = 0; i < A.size(); ++i) A[i] = rnd() * (1.f + (i % 7)) ;
    std::vector<int32_t> tiles;
    for (int r = 0; r < M; r += 128) { tiles.push_back(0); tiles.push_back(r); tiles.push_back(std::min(128, M - r)); }
    float *dA, *dW, *dC, *dBias; uint16_t* dBt; int32_t* dT;
    CK(hipMalloc(&dA, A.size() * 4)); CK(hipMalloc(&dW, W.size() * 4)); CK(hipMalloc(&dC, (size_t)M * N * 4)); CK(hipMalloc(&dBias, N * 4));
    CK(hipMalloc(&dBt, (size_t)3 * N * K * 2)); CK(hipMalloc(&dT, tiles.size() * 4));
    CK(hipMemcpy(dA, A.data(), A.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dW, W.data(), W.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dBias, bias.data(), N * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dT, tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_split_w, dim3((K + 31) / 32, (N + 31) / 32, 1), dim3(256), 0, 0, dW, 0, 0, K, N, 0, dBt, 3, gm_no_bound());
    SplitGemmK g{};
    g.A = dA; g.lda = K; g.Bt = dBt; g.bt_stride = 0; g.C = dC; g.ldc = N; g.K = K; g.N = N; g.bias = dBias; g.relu = 0;
    g.tiles = dT; g.n_tiles = (int)tiles.size() / 3; g.n_col_tiles = 1; g.nt_store = getenv("GS_NT") ? atoi(getenv("GS_NT")) : 1;
    auto launch = [&]() {
        if (half) hipLaunchKernelGGL((k_gemm_split_p<false, 1>), dim3(std::min(2 * g.n_tiles, cap)), dim3(1024), 0, 0, g);
        else hipLaunchKernelGGL((k_gemm_split_p<false, 2>), dim3(std::min(g.n_tiles, cap)), dim3(1024), 0, 0, g);
    };
    launch();
    CK(hipDeviceSynchronize());
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int reps = 20;
    float ms;
    const int sleep_us = getenv("GS_SLEEP_US") ? atoi(getenv("GS_SLEEP_US")) : 0;
    if (sleep_us > 0) {
        // "cool chip" mode: one launch at a time with a pause in between (inside the meta-step the GEMMs alternate with memory-bound kernels
        // and the part holds ~2 GHz; back to back it throttles to ~1.4 GHz), median of the per-launch times
        std::vector<float> t;
        for (int i = 0; i < reps; ++i) {
            usleep(sleep_us);
            CK(hipEventRecord(e0, 0)); launch(); CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
            float m1; CK(hipEventElapsedTime(&m1, e0, e1)); t.push_back(m1);
        }
        std::sort(t.begin(), t.end()); ms = t[t.size() / 2];
        printf("cool-chip mode (pause %d us): min %.3f median %.3f max %.3f ms\n", sleep_us, t.front(), ms, t.back());
    } else {
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < reps; ++i) launch();
        CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1)); ms /= reps;
    }
    const double fl = 2.0 * M * K * N;
    printf("split-bf16 GEMM: %.3f ms  %.1f TFLOP/s (fp32-equivalent)  %.1f TFLOP/s of bf16 MFMA work  %.2f TB/s of A+C traffic\n", ms, fl / ms / 1e9,
           6 * fl / ms / 1e9, ((double)M * K * 4 + (double)M * N * 4) / ms / 1e9);
    std::vector<float> C((size_t)M * N);
    CK(hipMemcpy(C.data(), dC, C.size() * 4, hipMemcpyDeviceToHost));
    // accuracy on a sample of rows: vs fp64, next to the fp32 fmaf chain's own error
    double e_split = 0, e_f32 = 0, mag = 0;
    for (int s = 0; s < 256; ++s) {
        const int row = (int)(((int64_t)s * 7919 * 131) % M);
        for (int n = 0; n < N; ++n) {
            double ref = 0; float f = 0.f;
            for (int k = 0; k < K; ++k) { ref += (double)A[(size_t)row * K + k] * (double)W[(size_t)k * N + n]; f = fmaf(A[(size_t)row * K + k], W[(size_t)k * N + n], f); }
            ref += bias[n]; f += bias[n];
            e_split = fmax(e_split, fabs((double)C[(size_t)row * N + n] - ref)); e_f32 = fmax(e_f32, fabs((double)f - ref)); mag = fmax(mag, fabs(ref));
        }
    }
    printf("max |C - fp64| over 256 rows: split-bf16 %.3e   fp32 fmaf chain %.3e   (max |C| %.3f)\n", e_split, e_f32, mag);
    return e_split < 20 * e_f32 + 1e-6 ? 0 : 2;
}
