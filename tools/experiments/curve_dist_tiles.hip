// curve_dist_tiles.hip -- the register tile of K20's tile kernel (statdepth_amd/csrc/curve_dist.hip), measured at
// 4 x 4, 8 x 4 and 8 x 8 accumulators per thread on the same data.  A stand-alone program, not part of the library:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off curve_dist_tiles.hip -o curve_dist_tiles && ./curve_dist_tiles
// Each variant is the product kernel's main loop with the store epilogue (256 threads as 16 x 16, panels of 16 timepoints
// in LDS, d = a - b; acc = fma(d, d, acc)); the tile is 16 RM targets x 16 RN curves.  Prints ms per n x n matrix and the
// share of 39.3e12 fp64 vector operations a second at 2 operations per pair-timepoint.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                    \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                     \
            std::printf("%s: %s\n", #x, hipGetErrorString(e_));                     \
            return 1;                                                               \
        }                                                                           \
    } while (0)

constexpr int TK = 16;

template <int RM, int RN>
__global__ __launch_bounds__(256, 2) void tile_kernel(const double *__restrict__ Y, long T, long n, long nb, double *__restrict__ out) {
    constexpr int BM = 16 * RM, BN = 16 * RN;
    __shared__ __attribute__((aligned(16))) double As[TK][BM];
    __shared__ __attribute__((aligned(16))) double Bs[TK][BN];
    const int tid = threadIdx.x, x = tid & 15, y = tid >> 4;
    const long q0 = (long)blockIdx.x / nb * BM, j0 = (long)blockIdx.x % nb * BN;
    double acc[RM][RN];
#pragma unroll
    for (int r = 0; r < RM; ++r)
#pragma unroll
        for (int c = 0; c < RN; ++c) acc[r][c] = 0.0;
    for (long t0 = 0; t0 < T; t0 += TK) {
        __syncthreads();
        for (int i = tid; i < TK * BM; i += 256) {
            const long t = t0 + i / BM, q = q0 + i % BM;
            As[i / BM][i % BM] = t < T && q < n ? Y[t * n + q] : 0.0;
        }
        for (int i = tid; i < TK * BN; i += 256) {
            const long t = t0 + i / BN, j = j0 + i % BN;
            Bs[i / BN][i % BN] = t < T && j < n ? Y[t * n + j] : 0.0;
        }
        __syncthreads();
        const int rows = T - t0 < TK ? (int)(T - t0) : TK;
#pragma unroll 2
        for (int k = 0; k < rows; ++k) {
            double a[RM], b[RN];
#pragma unroll
            for (int r = 0; r < RM; r += 2) {
                const double2 v = *reinterpret_cast<const double2 *>(&As[k][RM * y + r]);
                a[r] = v.x, a[r + 1] = v.y;
            }
#pragma unroll
            for (int c = 0; c < RN / 2; ++c) {
                const double2 v = *reinterpret_cast<const double2 *>(&Bs[k][32 * c + 2 * x]);
                b[2 * c] = v.x, b[2 * c + 1] = v.y;
            }
#pragma unroll
            for (int r = 0; r < RM; ++r)
#pragma unroll
                for (int c = 0; c < RN; ++c) {
                    const double d = a[r] - b[c];
                    acc[r][c] = fma(d, d, acc[r][c]);
                }
        }
    }
#pragma unroll
    for (int r = 0; r < RM; ++r) {
        const long q = q0 + RM * y + r;
#pragma unroll
        for (int c = 0; c < RN; ++c) {
            const long j = j0 + 32 * (c >> 1) + 2 * x + (c & 1);
            if (q < n && j < n) out[q * n + j] = acc[r][c];
        }
    }
}

template <int RM, int RN>
static int measure(const double *Y, long T, long n, double *out, double *first_row, std::vector<double> &row) {
    const long tb = (n + 16 * RM - 1) / (16 * RM), nb = (n + 16 * RN - 1) / (16 * RN);
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    float best = 1e30f;
    for (int rep = 0; rep < 6; ++rep) {
        CHECK(hipEventRecord(a));
        hipLaunchKernelGGL((tile_kernel<RM, RN>), dim3((unsigned)(tb * nb)), dim3(256), 0, 0, Y, T, n, nb, out);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        float ms;
        CHECK(hipEventElapsedTime(&ms, a, b));
        if (rep && ms < best) best = ms;
    }
    CHECK(hipMemcpy(row.data(), out + n, n * sizeof(double), hipMemcpyDeviceToHost));   // row 1, compared across the variants
    bool same = true;
    if (first_row)
        for (long j = 0; j < n; ++j) same = same && row[j] == first_row[j];
    std::printf("tile %d x %d (%3d x %3d curves): %8.3f ms  share of the fp64 vector peak %.3f  %s\n", RM, RN, 16 * RM, 16 * RN, best,
                2.0 * n * n * T / (best * 1e-3) / 39.3e12, first_row ? (same ? "same bits as the first" : "DIFFERENT BITS") : "");
    return 0;
}

int main(int argc, char **argv) {
    const long n = argc > 1 ? std::atol(argv[1]) : 10000, T = argc > 2 ? std::atol(argv[2]) : 1000;
    std::vector<double> X((size_t)T * n), r0(n), r1(n);
    unsigned long long s = 88172645463325252ull;
    for (auto &v : X) {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        v = (double)(s >> 11) / 9007199254740992.0 - 0.5;
    }
    double *Y, *out;
    CHECK(hipMalloc(&Y, X.size() * sizeof(double)));
    CHECK(hipMalloc(&out, (size_t)n * n * sizeof(double)));
    CHECK(hipMemcpy(Y, X.data(), X.size() * sizeof(double), hipMemcpyHostToDevice));
    std::printf("n = %ld curves, T = %ld timepoints\n", n, T);
    if (measure<8, 8>(Y, T, n, out, nullptr, r0)) return 1;
    if (measure<8, 4>(Y, T, n, out, r0.data(), r1)) return 1;
    if (measure<4, 8>(Y, T, n, out, r0.data(), r1)) return 1;
    if (measure<4, 4>(Y, T, n, out, r0.data(), r1)) return 1;
    CHECK(hipFree(Y));
    CHECK(hipFree(out));
    return 0;
}
