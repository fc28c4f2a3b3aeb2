// simplex_retired.hip -- the generic (scratch-memory) generation of the K4 kernels (simplex.hip), linked into
// libstatdepth_hip_xcheck.so alone: an independent implementation for the parity tests, reached through
// retired_simplex_generic (sd_common.h) when SD_SIMPLEX_GENERIC = 1.  The product library holds neither the kernel nor
// a way to ask for it.  The hull test from the data, the subsets and the work split are the product's (simplex_hull.h;
// the grid: launch_simplex_common).
#include "simplex_hull.h"

namespace sd {

// grid = (chunks, m).  T == 0 selects the pointcloud form (P is n x d);
// otherwise P is n x T x d and c counts timepoints (relax / strict reduction).
__global__ __launch_bounds__(SX_THREADS) void simplex_kernel(
    const double *__restrict__ P, i64 n, i64 T, int d, PointSel sel, int relax, double tol,
    u64 total, u64 per_thread, i64 samples, u64 seed, i64 q0, u64 *__restrict__ out) {
    __shared__ u64 scratch[SX_THREADS / 64];
    i64 q = q0 + blockIdx.y;
    int k = d + 1;
    const PointView blk = point_view(sel, P, n, d, q);
    const i64 tg = blk.tg, no = blk.others();
    const bool direct = sx_direct(blk, samples);
    total = sx_total(blk, k, total);
    u64 tid = (u64)blockIdx.x * SX_THREADS + threadIdx.x;
    u64 first = tid * per_thread;
    u64 acc = 0;
    if (first < total) {
        u64 last = first + per_thread < total ? first + per_thread : total;
        i64 idx[SMAX];
        double pts[SMAX * 8], x[8];
        if (samples < 0) unrank_comb(first, k, no, idx);
        u64 snext = 0;                                                  // sampled: the shared index behind the last subset taken
        if (samples >= 0)
            for (u64 r = 0; r < first; ++r) sample_next_valid(seed, tg, &snext, k, n, idx);   // this thread's first valid subset
        i64 TT = T > 0 ? T : 1;
        for (u64 r = first; r < last; ++r) {
            if (samples >= 0) sample_next_valid(seed, tg, &snext, k, n, idx);
            u64 cnt = 0;
            for (i64 t = 0; t < TT; ++t) {
                for (int c = 0; c < k; ++c) {
                    i64 src = sx_src(blk, direct, idx[c]);
                    const double *pp = P + (src * TT + t) * d;
                    for (int e = 0; e < d; ++e) pts[c * d + e] = pp[e];
                }
                const double *xx = T > 0 ? P + (tg * TT + t) * d : blk.x;  // curves (rows form only): the target at timepoint t
                for (int e = 0; e < d; ++e) x[e] = xx[e];
                cnt += point_in_hull(pts, k, d, x, tol);
            }
            acc += (T > 0 && !relax) ? (cnt / (u64)TT) : cnt;
            if (samples < 0 && r + 1 < last) next_comb(idx, k, no);
        }
    }
    u64 tot = block_sum_u64(acc, scratch);
    if (threadIdx.x == 0 && tot) atomicAdd(&out[q], tot);
}

int retired_simplex_generic(const double *P, i64 n, i64 T, int d, const PointSel &sel, int relax, double tol, u64 total,
                            u64 per_thread, i64 samples, u64 seed, i64 q0, u64 *out, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL(simplex_kernel, grid, dim3(SX_THREADS), 0, s, P, n, T, d, sel, relax, tol, total, per_thread, samples, seed,
                       q0, out);
    return SD_OK;
}

}  // namespace sd
