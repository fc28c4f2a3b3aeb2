// oja.hip -- K7: Oja volume sums of a point cloud.
//
// Replaces the subset loop of _oja_depth (_pointcloud.py:175-205; one scipy ConvexHull per simplex) with
//   out[q] = sum over d-subsets S of the target's others of |det[x_s1 - x, ..., x_sd - x]| / d!
// (the volume of conv(S u {x})).  The host divides by ConvexHull(sample).volume.
//
// Work decomposition (the K4 scheme): a target's C(no, d) subsets, in lexicographic order, are cut into ranges of
// OJA_PER_THREAD subsets; 256 consecutive ranges form a SLICE, one workgroup per (target, slice).  The range length is a
// constant, so a workgroup's work is bounded whatever no is; a large target has many slices instead.  A thread
// unranks its first subset once and then steps.  The last index varies fastest and det[A | a_k] is linear in a_k:
// det = c . a_k with c the cofactor vector of the d - 1 prefix columns (a_i = x_i - x), recomputed only when the
// prefix changes.  The inner loop is d multiplies, d - 1 adds, an abs and an add.
//
// The translated others (x_k - x) sit in LDS when no * d * 8 bytes fit OJA_LDS_MAX (all sizes of the tools/time_oja.py
// table), else they are read from global memory and translated on the fly -- the same fp64 operations, so the same bits.
//
// Determinism: ranges and slices depend only on (no, d); a thread sums its range in order; a slice is reduced in a
// fixed tree; slices are folded into out[q] strictly in slice order by oja_fold_kernel.  So a target's result does
// not depend on m, on the other targets of the call, or on how the call is cut into launches.  No atomics.
#include "sd_common.h"
#include "point_select.h"

namespace sd {

constexpr int OJA_THREADS = 256;
constexpr size_t OJA_LDS_MAX = 64 * 1024;                         // translated others in LDS up to this size
constexpr u64 OJA_PER_THREAD = 128;                              // subsets per thread (the unrank and the LDS fill amortised)
constexpr u64 OJA_SLICE = OJA_PER_THREAD * OJA_THREADS;           // subsets per workgroup: 32 768
// subset evaluations per launch: 2^32 up to d = 5, halved per dimension above; every workgroup holds at most OJA_SLICE of
// them, so a launch is at least min(units, 2^29 / 32 768 = 16 384) workgroups and its duration is bounded by the cap
// (tools/time_oja.py on one MI355X: longest launch 9.5 / 19 / 14 ms at d = 2 / 5 / 8; profiles/oja_profile.json)
constexpr u64 OJA_LAUNCH_EVALS = (u64)1 << 32;

// C(a, k) for k <= 8; the divisors are constants once the loop is unrolled.  Callers keep k * C(a, k) < 2^64.
__host__ __device__ __forceinline__ u64 oja_binom(u64 a, int k) {
    if (k < 0 || (u64)k > a) return 0;
    u64 c = 1;
#pragma unroll
    for (int j = 1; j <= 8; ++j)
        if (j <= k) c = c * (a - (u64)j + 1) / (u64)j;
    return c;
}

__host__ __device__ __forceinline__ u64 oja_slices(u64 total) { return (total + OJA_SLICE - 1) / OJA_SLICE; }

// lexicographic unranking of the r-th K-subset of {0..no-1}: per position a binary search on
// #{subsets whose element at this position is < c} = C(no - c0, kk) - C(no - c, kk)
template <int K>
__device__ static void oja_unrank(u64 r, i64 no, int *idx) {
    i64 c0 = 0;
#pragma unroll
    for (int p = 0; p < K; ++p) {
        const int kk = K - p;
        const u64 all = oja_binom((u64)(no - c0), kk);
        const u64 need = all - r;                                   // largest c with C(no - c, kk) >= need
        i64 lo = c0, hi = no - kk;
        while (lo < hi) {
            const i64 mid = lo + (hi - lo + 1) / 2;
            if (oja_binom((u64)(no - mid), kk) >= need) lo = mid;
            else hi = mid - 1;
        }
        r -= all - oja_binom((u64)(no - lo), kk);
        idx[p] = (int)lo;
        c0 = lo + 1;
    }
}

// translated other i: from LDS, or read and translated here (the same subtraction either way)
template <int D>
__device__ __forceinline__ void oja_row(const double *lds, const double *P, const PointView &b, const double *x, i64 i,
                                        double (&a)[D]) {
    if (lds) {
#pragma unroll
        for (int e = 0; e < D; ++e) a[e] = lds[i * D + e];
    } else {
        const double *p = P + b.other(i) * D;
#pragma unroll
        for (int e = 0; e < D; ++e) a[e] = p[e] - x[e];
    }
}

// c with det[a_0 | ... | a_{D-2} | y] = c . y for every y
template <int D>
__device__ __forceinline__ void oja_cofactor(const double (&A)[D > 1 ? D - 1 : 1][D], double (&c)[D]) {
    if constexpr (D == 1) {
        c[0] = 1.0;
    } else if constexpr (D == 2) {
        c[0] = -A[0][1];
        c[1] = A[0][0];
    } else if constexpr (D == 3) {
        c[0] = A[0][1] * A[1][2] - A[0][2] * A[1][1];
        c[1] = A[0][2] * A[1][0] - A[0][0] * A[1][2];
        c[2] = A[0][0] * A[1][1] - A[0][1] * A[1][0];
    } else {
        // P M = L U with partial pivoting, M = [a_0 .. a_{D-2}] (D x (D-1), rows = coordinates).  Then
        // det[M | y] = sgn(P) * prod(U_jj) * (l . P y) with L^T l = e_{D-1}: c[perm[i]] = sgn * prod * l[i].
        constexpr int C = D - 1;
        double M[D][C];
        int perm[D];
#pragma unroll
        for (int r = 0; r < D; ++r) {
            perm[r] = r;
#pragma unroll
            for (int j = 0; j < C; ++j) M[r][j] = A[j][r];
        }
        double prod = 1.0;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            int p = j;
            double best = fabs(M[j][j]);
#pragma unroll
            for (int r = j + 1; r < D; ++r)
                if (fabs(M[r][j]) > best) { best = fabs(M[r][j]); p = r; }
            if (best == 0.0) {                                      // rank deficient prefix: every determinant is 0
#pragma unroll
                for (int e = 0; e < D; ++e) c[e] = 0.0;
                return;
            }
            if (p != j) {
                prod = -prod;
#pragma unroll
                for (int r = j + 1; r < D; ++r)
                    if (r == p) {
#pragma unroll
                        for (int k = 0; k < C; ++k) { const double t = M[j][k]; M[j][k] = M[r][k]; M[r][k] = t; }
                        const int t = perm[j]; perm[j] = perm[r]; perm[r] = t;
                    }
            }
            prod *= M[j][j];
#pragma unroll
            for (int r = j + 1; r < D; ++r) {
                const double f = M[r][j] / M[j][j];
                M[r][j] = f;                                        // L's multiplier, kept in place (swapped with its row)
#pragma unroll
                for (int k = j + 1; k < C; ++k) M[r][k] -= f * M[j][k];
            }
        }
        double l[D];
        l[D - 1] = 1.0;
#pragma unroll
        for (int i = D - 2; i >= 0; --i) {
            double s = 0.0;
#pragma unroll
            for (int r = i + 1; r < D; ++r) s += M[r][i] * l[r];
            l[i] = -s;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double v = prod * l[i];
#pragma unroll
            for (int e = 0; e < D; ++e)
                if (perm[i] == e) c[e] = v;
        }
    }
}

__device__ __forceinline__ double oja_block_sum(double v, double *scratch) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < OJA_THREADS / 64; ++k) r += scratch[k];
    return r;
}

// one workgroup per work unit u = u0 + blockIdx.x = (target q = u / S, slice s = u % S); part[blockIdx.x] = the slice's sum
template <int D>
__global__ __launch_bounds__(OJA_THREADS) void oja_kernel(const double *__restrict__ P, i64 n, PointSel sel, u64 u0, u64 S,
                                                          int use_lds, double *__restrict__ part) {
    extern __shared__ double oja_lds[];
    __shared__ double scratch[OJA_THREADS / 64];
    const u64 u = u0 + blockIdx.x;
    const i64 q = (i64)(u / S);
    const u64 s = u % S;
    const PointView b = point_view(sel, P, n, D, q);        // the subsets come from the target's others (point_select.h)
    const i64 no = b.others();
    const u64 total = oja_binom((u64)no, D);
    constexpr u64 L = OJA_PER_THREAD;
    if (s >= oja_slices(total)) {                                   // a smaller block of the members form
        if (threadIdx.x == 0) part[blockIdx.x] = 0.0;
        return;
    }
    double x[D];
#pragma unroll
    for (int e = 0; e < D; ++e) x[e] = b.x[e];
    const double *lds = nullptr;
    if (use_lds) {
        for (i64 i = threadIdx.x; i < no; i += OJA_THREADS) {
            const double *p = P + b.other(i) * D;
#pragma unroll
            for (int e = 0; e < D; ++e) oja_lds[i * D + e] = p[e] - x[e];
        }
        __syncthreads();
        lds = oja_lds;
    }
    const u64 first = (s * OJA_THREADS + threadIdx.x) * L;
    double acc = 0.0;
    if (first < total) {
        u64 left = total - first < L ? total - first : L;
        int idx[D];
        oja_unrank<D>(first, no, idx);
        for (;;) {
            double c[D];
            if constexpr (D == 1) {
                c[0] = 1.0;
            } else {
                double A[D - 1][D];
#pragma unroll
                for (int j = 0; j < D - 1; ++j) oja_row<D>(lds, P, b, x, idx[j], A[j]);
                oja_cofactor<D>(A, c);
            }
            const i64 k0 = idx[D - 1];
            const u64 run = (u64)(no - k0) < left ? (u64)(no - k0) : left;
            for (u64 j = 0; j < run; ++j) {
                double a[D];
                oja_row<D>(lds, P, b, x, k0 + (i64)j, a);
                double v = c[0] * a[0];
#pragma unroll
                for (int e = 1; e < D; ++e) v += c[e] * a[e];
                acc += fabs(v);
            }
            left -= run;
            if (left == 0) break;
            if constexpr (D == 1) {
                break;                                              // (a range never outruns the only index)
            } else {                                                // next prefix of D - 1 indices that leaves room for the last
                int i = 0;                                          // the rightmost prefix position below its maximum
#pragma unroll
                for (int t = 0; t < D - 1; ++t)
                    if (idx[t] != (int)no - D + t) i = t;
#pragma unroll
                for (int t = 0; t < D - 1; ++t) {
                    if (t == i) ++idx[t];
                    else if (t > i) idx[t] = idx[t - 1] + 1;
                }
                idx[D - 1] = idx[D - 2] + 1;
            }
        }
    }
    const double tot = oja_block_sum(acc, scratch);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// fold the slice sums of units [u0, u1) into out[q], in slice order; a target whose last slice is in the range is
// divided by d! (out holds the raw running sum between launches)
__global__ __launch_bounds__(256) void oja_fold_kernel(const double *__restrict__ part, u64 u0, u64 u1, u64 S, double fact,
                                                       double *__restrict__ out) {
    const i64 q = (i64)(u0 / S) + (i64)blockIdx.x * 256 + threadIdx.x;
    const u64 qb = (u64)q * S, qe = qb + S;
    if (qb >= u1) return;
    const u64 a = qb > u0 ? qb : u0, e = qe < u1 ? qe : u1;
    double acc = a == qb ? 0.0 : out[q];
    u64 u = a;
    for (; u + 8 <= e; u += 8) {                                    // loads issued together, added in order
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = part[u - u0 + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += v[k];
    }
    for (; u < e; ++u) acc += part[u - u0];
    out[q] = e == qe ? acc / fact : acc;
}

template <int D>
static int launch_oja_d(const double *P, i64 n, const PointSel &sel, i64 m, double *out, hipStream_t s) {
    const i64 no_max = sel_others_max(sel, n);
    const u64 total = oja_binom((u64)no_max, D);
    if (total == 0) {                                               // fewer than d others everywhere: empty sums
        SD_HIP(hipMemsetAsync(out, 0, sizeof(double) * m, s));
        return SD_OK;
    }
    const u64 S = oja_slices(total);
    const u64 units = (u64)m * S;
    u64 per_launch = (OJA_LAUNCH_EVALS >> (D > 5 ? D - 5 : 0)) / OJA_SLICE;
    if (per_launch > units) per_launch = units;
    const size_t lds_bytes = (size_t)no_max * D * sizeof(double);
    const int use_lds = lds_bytes <= OJA_LDS_MAX ? 1 : 0;
    if (use_lds)
        SD_HIP(hipFuncSetAttribute((const void *)oja_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    double fact = 1.0;
    for (int k = 2; k <= D; ++k) fact *= (double)k;
    double *part = nullptr;
    SD_HIP(hipMallocAsync((void **)&part, per_launch * sizeof(double), s));
    hipError_t err = hipSuccess;
    for (u64 u0 = 0; u0 < units && err == hipSuccess; u0 += per_launch) {
        const u64 cnt = units - u0 < per_launch ? units - u0 : per_launch;
        hipLaunchKernelGGL((oja_kernel<D>), dim3((unsigned)cnt), dim3(OJA_THREADS), use_lds ? lds_bytes : 0, s, P, n, sel, u0,
                           S, use_lds, part);
        err = hipGetLastError();
        if (err != hipSuccess) break;
        const u64 q0 = u0 / S, q1 = (u0 + cnt - 1) / S;
        hipLaunchKernelGGL(oja_fold_kernel, dim3((unsigned)((q1 - q0 + 1 + 255) / 256)), dim3(256), 0, s, part, u0, u0 + cnt,
                           S, fact, out);
        err = hipGetLastError();
    }
    const hipError_t ferr = hipFreeAsync(part, s);                 // freed on the error path too
    if (err != hipSuccess)
        return fail(SD_ERR_HIP, "oja launch failed: %s (%s:%d)", hipGetErrorString(err), __FILE__, __LINE__);
    SD_HIP(ferr);
    return SD_OK;
}

int launch_oja(const double *P, i64 n, int d, const PointSel &sel, i64 m, double *out, hipStream_t s) {
    SD_DISPATCH_D(d, return launch_oja_d<D_>(P, n, sel, m, out, s))
    return fail(SD_ERR_UNSUPPORTED, "oja volume sums cover d in [1,8], got %d", d);
}

}  // namespace sd
