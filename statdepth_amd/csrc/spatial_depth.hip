// spatial_depth.hip -- K21: the functional spatial depth of curves (Chakraborty & Chaudhuri 2014; Sguera, Galeano & Lillo 2014;
// depth.FSD of fda.usc), FSD(x) = 1 - |(1/N) sum_j (x - x_j) / |x - x_j||, L2 norms over a uniform time grid.
//
// Definition.  n curves at T timepoints, time-major Y[t][j], finite, |y| <= 2^480.  For a target x (a sample curve, or an
// external curve, a column of Q):
//   D2[j]  K20's squared distance on K20's bits (curve_dist.hip): one accumulator over ascending t from +0.0,
//          d = x[t] - Y[t][j]; acc = fma(d, d, acc);
//   w[j]   0.0 where D2[j] == 0.0, else 1.0 / sqrt(D2[j]): a correctly rounded root, then one correctly rounded division
//          (pass 1: the tile kernel's epilogue CD_WEIGHT);
//   E[t]   per timepoint one accumulator over ascending j = 0 .. n - 1 from +0.0:
//          d = x[t] - Y[t][j]; E = fma(w[j], d, E)                                          (pass 2: sp_sum_kernel);
//   S      one accumulator over ascending t from +0.0: S = fma(E[t], E[t], S)               (sp_fold_kernel).
// out = S; the host forms depth = 1 - sqrt(S) / N, N = n for a sample target and n + 1 for an external one.
// A coincident curve (D2 == 0: the target's own column, a duplicate, or differences whose every square underflows inside
// the fma) has weight 0, adds nothing and still counts in N: the papers' sum over x_j != x.  K5 (l1_depth.hip) returns NaN
// there because its reference does; this kernel differs on purpose.  No target index is special-cased.
// The sum over j is the direct form and is never split: no Gram form x sum w - sum w_j x_j (it cancels for curves that are
// close relative to their level), no matrix instructions (fp64 MFMA has no rate advantage over fp64 FMA on gfx950 and would
// force the Gram form), no floating-point atomics.  E and S of a target hold the same bits whatever the target list, the
// tiles, the layout of X or the workspace.
//
// sp_sum_kernel<C>: one workgroup of 256 threads per (128 targets x 16 C timepoints) walks all n sample curves in ascending
// j, in chunks of 16 staged through LDS: the weight panel [j][q] as pass 1 wrote it (a straight copy, 16 KiB), and the sample
// panel [j][t], transposed while staging from the time-major Y (whose rows keep j contiguous); its rows are padded by one
// double (16 C + 1), so the 16 lanes that write one timepoint of 16 curves hit 16 different bank pairs and the 16 lanes
// that read 16 timepoints of one curve read 128 consecutive bytes.  Thread (x, y) = (tid & 15, tid >> 4) holds the targets
// 8 y + r and the timepoints 16 c + x: a register tile of 8 x C accumulators and as many of the targets' own values x[q][t],
// constant over the j loop.  Per j and element one subtraction and one fma, K20's instruction mix (curve_dist.hip on the tile
// shape and the LDS bytes per operation): 8 weights and C samples read from LDS per 8 C elements.
// C = 4 (128 x 64) is the tile; where it would give the device fewer than two workgroups per CU the launcher takes C = 2
// (128 x 32: twice the workgroups, 12 doubles read per 16 elements).  The bits do not depend on the choice.  j is never split.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), no scratch and no spill in any of them:
//   sp_sum_kernel<4>  218 VGPRs, 2 waves a SIMD, 24 704 B of LDS    (64 + 64 for the two register tiles, 16 + 2 C for the
//   sp_sum_kernel<2>  142 VGPRs, 3 waves a SIMD, 20 608 B of LDS     next chunk in flight)
//   sp_fold_kernel      8 VGPRs, 8 waves a SIMD
// The next chunk is fetched into registers while the chunk at hand is consumed: the weights stream from memory (8 n bytes a
// target, each byte read by every time tile of its block) where K20's panels sit in the caches, and only two or three
// workgroups share a CU, so the latency of a chunk's loads has to lie behind the arithmetic of the chunk before.  Measured
// at 10 000 x 1 000: pass 2 takes 9.14 ms against 7.94 ms of the distance pass in the same run (DESIGN section 3 K21;
// profiles/spatial_depth_times.txt).  Bounding <4> to 3 waves a SIMD (168 VGPRs) spills registers to scratch; it stays at 2.
// The batch plan (spatial_plan), in the blocks of curve_routes.h: the weights of a batch, n x targets doubles, and its field,
// targets x T doubles (with `field` given the kernel writes there and the plan's part stays unused).  The recommended size
// holds all targets up to SP_WEIGHTS_MAX = 8 GiB of weights: at 100 000 x 256 that is 83 blocks a batch, 664 workgroups of
// pass 2 at C = 2, more than two for each of the 256 CUs (1 GiB would give 10 blocks, 80 workgroups).
#include "curve_routes.h"

namespace sd {

constexpr int SP_TILE = CV_BLOCK;                                   // targets of a tile: the blocks of the plan, pass 1's tile
constexpr int SP_JK = 16, SP_THREADS = 256, SP_R = SP_TILE / 16;    // sample curves of a chunk; targets of a thread
constexpr size_t SP_WEIGHTS_MAX = (size_t)8 << 30;                  // weights of a batch (recommended size and launch)

// Targets [q_first + 128 (blockIdx.x / tt) ...) x timepoints [16 C (blockIdx.x % tt) ...).  P, ldp, targets: the targets'
// panel, value (t, q) = P[t * ldp + (targets ? targets[q] : q)].  q_end: one past the last target.  row0: the batch's first
// target; W[j * ldw + (q - row0)]; E[(q - row0) * lde + t].
template <int C>
__global__ __launch_bounds__(SP_THREADS, 2) void sp_sum_kernel(const double *__restrict__ Y, i64 T, i64 n, const double *__restrict__ P,
                                                            i64 ldp, const i64 *__restrict__ targets, i64 q_first, i64 q_end, i64 tt,
                                                            i64 row0, const double *__restrict__ W, i64 ldw, double *__restrict__ E,
                                                            i64 lde) {
    constexpr int TT = 16 * C;
    __shared__ __attribute__((aligned(16))) double Ws[SP_JK][SP_TILE];
    __shared__ double Ys[SP_JK][TT + 1];
    const int tid = threadIdx.x, x = tid & 15, y = tid >> 4;
    const i64 q0 = q_first + (i64)blockIdx.x / tt * SP_TILE, t0 = (i64)blockIdx.x % tt * TT;

    // the targets' own values and the accumulators
    double xq[SP_R][C], acc[SP_R][C];
#pragma unroll
    for (int r = 0; r < SP_R; ++r) {
        const i64 q = q0 + SP_R * y + r;
        const double *p = q < q_end ? P + (targets ? targets[q] : q) : nullptr;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const i64 t = t0 + 16 * c + x;
            xq[r][c] = p && t < T ? p[t * ldp] : 0.0;
            acc[r][c] = 0.0;
        }
    }

    // a thread fetches one column of the weight panel at the rows (tid >> 7) + 2 l of a chunk, and of the sample panel the
    // curve tid & 15 at the timepoints (tid >> 4) + 16 l; the next chunk is fetched into registers before the chunk at hand
    // is consumed, so its latency lies behind the arithmetic
    const int col = tid & (SP_TILE - 1), k0 = tid >> 7;
    const double *pw = W + (q0 - row0) + col;
    double fw[SP_JK / 2], fy[C];
    auto fetch = [&](i64 j0) {
#pragma unroll
        for (int l = 0; l < SP_JK / 2; ++l) {
            const i64 j = j0 + k0 + 2 * l;
            fw[l] = j < n ? pw[j * ldw] : 0.0;
        }
#pragma unroll
        for (int l = 0; l < C; ++l) {
            const i64 j = j0 + x, t = t0 + y + 16 * l;
            fy[l] = j < n && t < T ? Y[t * n + j] : 0.0;
        }
    };
    fetch(0);
    for (i64 j0 = 0; j0 < n; j0 += SP_JK) {
        __syncthreads();                                            // the chunk before is consumed
#pragma unroll
        for (int l = 0; l < SP_JK / 2; ++l) Ws[k0 + 2 * l][col] = fw[l];
#pragma unroll
        for (int l = 0; l < C; ++l) Ys[x][y + 16 * l] = fy[l];
        __syncthreads();
        if (j0 + SP_JK < n) fetch(j0 + SP_JK);
        const int rows = n - j0 < SP_JK ? (int)(n - j0) : SP_JK;
#pragma unroll 2
        for (int k = 0; k < rows; ++k) {
            double a[SP_R], b[C];
#pragma unroll
            for (int r = 0; r < SP_R; r += 2) {
                const double2 v = *reinterpret_cast<const double2 *>(&Ws[k][SP_R * y + r]);
                a[r] = v.x, a[r + 1] = v.y;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) b[c] = Ys[k][16 * c + x];
#pragma unroll
            for (int r = 0; r < SP_R; ++r)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const double d = xq[r][c] - b[c];
                    acc[r][c] = fma(a[r], d, acc[r][c]);
                }
        }
    }

#pragma unroll
    for (int r = 0; r < SP_R; ++r) {
        const i64 q = q0 + SP_R * y + r;
        if (q >= q_end) continue;
        double *row = E + (q - row0) * lde;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const i64 t = t0 + 16 * c + x;
            if (t < T) row[t] = acc[r][c];
        }
    }
}

// out[q] = the squared norm of row q of E over ascending t
__global__ __launch_bounds__(256) void sp_fold_kernel(const double *__restrict__ E, i64 count, i64 T, i64 lde, double *__restrict__ out) {
    const i64 q = (i64)blockIdx.x * 256 + threadIdx.x;
    if (q >= count) return;
    const double *e = E + q * lde;
    double s = 0.0;
    for (i64 t = 0; t < T; ++t) s = fma(e[t], e[t], s);
    out[q] = s;
}

// ---------------------------------------------------------------------------------------------- the batch plan
SpatialPlan spatial_plan(i64 T, i64 n, i64 m, PlanSize size) {
    SpatialPlan p{0, 0, 0, 0};
    const size_t wb = (size_t)SP_TILE * (size_t)n * 8, fb = (size_t)SP_TILE * (size_t)T * 8;   // of 128 targets; multiples of 256
    const TargetBlocks b = target_block_plan(m, size, wb + fb, wb, SP_WEIGHTS_MAX);
    if (b.blocks < 1) return p;
    p.targets = b.targets;
    p.weights = (size_t)b.blocks * wb;
    p.field = (size_t)b.blocks * fb;
    p.bytes = p.weights + p.field;
    return p;
}

int spatial_time_tile(i64 T, i64 targets, i64 cus) {
    const i64 wide = (targets + SP_TILE - 1) / SP_TILE * ((T + 63) / 64);   // workgroups of the 128 x 64 tile
    return wide >= 2 * cus ? 64 : 32;
}

// ---------------------------------------------------------------------------------------------- host
template <int C>
static int sp_launch_tiles(const double *Y, i64 T, i64 n, CurveSel sel, i64 m, i64 q_begin, i64 q_end, const double *W, i64 ldw,
                           double *E, hipStream_t s) {
    const i64 tt = (T + 16 * C - 1) / (16 * C);                     // time tiles of a target block
    return for_block_launches(q_begin, q_end, tt, [&](i64 q, i64 tb) -> int {
        hipLaunchKernelGGL(sp_sum_kernel<C>, dim3((unsigned)(tb * tt)), dim3(SP_THREADS), 0, s, Y, T, n, sel.panel(Y), sel.ld(n, m),
                           sel.targets, q, q_end, tt, q_begin, W, ldw, E, T);
        SD_HIP(hipGetLastError());
        return SD_OK;
    });
}

int launch_spatial_sums(const double *Y, i64 T, i64 n, CurveSel sel, i64 m, double *out, double *field, void *ws, size_t ws_bytes,
                        hipStream_t s) {
    const SpatialPlan plan = spatial_plan(T, n, m, PlanSize::of_bytes(ws_bytes));
    Carver cv(ws, ws_bytes);
    double *W = plan.targets > 0 ? (double *)cv.take(plan.weights) : nullptr;
    double *F = W ? (double *)cv.take(plan.field) : nullptr;
    if (!W || !F) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_spatial_min_workspace_bytes)");
    const i64 ldw = (plan.targets + SP_TILE - 1) / SP_TILE * SP_TILE, cus = stream_cus(s);
    return for_target_batches(m, plan.targets, [&](i64 q, i64 count) -> int {
        int rc = launch_curve_weights(Y, T, n, sel, m, q, q + count, W, ldw, s);
        if (rc) return rc;
        double *E = field ? field + q * T : F;
        rc = spatial_time_tile(T, count, cus) == 64 ? sp_launch_tiles<4>(Y, T, n, sel, m, q, q + count, W, ldw, E, s)
                                                    : sp_launch_tiles<2>(Y, T, n, sel, m, q, q + count, W, ldw, E, s);
        if (rc) return rc;
        hipLaunchKernelGGL(sp_fold_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, E, count, T, T, out + q);
        SD_HIP(hipGetLastError());
        return SD_OK;
    });
}

}  // namespace sd
