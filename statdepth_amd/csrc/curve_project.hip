// curve_project.hip -- K23: the projections of curves on a fixed set of directions, and the random projection depths built
// on them (random projection depth of Cuevas, Febrero & Fraiman 2007, random Tukey depth of Cuesta-Albertos & Nieto-Reyes
// 2008, Stahel-Donoho outlyingness over the same projections).
//
// Definition.  n curves at T timepoints, x(t, i) = X[t * st + i * sn] in either layout, finite; k directions, the rows of U
// (k x T, row-major).  For curve i and direction r, one accumulator over ascending t:
//   z = x_0 u_r0;   z = z + x_t u_rt   (t = 1 .. T - 1)
// every product and every sum rounded separately to fp64 (__dmul_rn, __dadd_rn: no FMA, no contraction), the first term the
// product alone and not 0 + product ((-0.0) stays -0.0).  For T <= 8 these are hs_proj<D>'s bits (K10, K12).  Z is k x n,
// Z[r][i], direction-major: a time-major matrix of k "timepoints", which is what K14's stage 1 and K10's row sort take.
//
// cp_project_kernel: one workgroup of 256 threads per (128 curves x 64 directions), K20's tile turned round.  Panels of 16
// timepoints of X (16 x 128) and of U (16 x 64) go through LDS, 16 + 8 KiB, every panel row padded by two doubles (16 640 +
// 8 448 bytes) so that the staging of a curve-major X and of U -- lanes along t, one LDS row each -- spreads over the
// banks.  Both layouts of X are read in place: time-major with the lanes along the curves, curve-major with the lanes along
// t; there is no transposed copy.  Thread (x, y) = (tid & 15, tid >> 4) holds a 4 x 8 register tile: the directions 4 y + c
// and the curves 32 g + 2 x + e, so a wave reads 16 consecutive 16-byte words of the X panel four times and two words of the
// U panel (broadcast over x), and stores runs of 16 x 16 bytes of a row of Z.  An accumulator belongs to one thread for the
// whole of t and there are no atomics: the bits of Z do not depend on the tiling, the layout or the launch shape.
// The last panel's tail rows are skipped (a zero-filled tail would turn -0.0 into +0.0); lanes past n or past the last
// direction stage zeros, compute on them and store nothing.  Every index that holds r n + i or t st + i sn is 64-bit.
// A launch covers at most CP_LAUNCH_GROUPS workgroups.
//
// The depths (sd_rp_depth_sums): a chunk of rows of Z goes to the workspace and launch_rank_depth_sums (K14) folds it into
// the records as it folds rows of curves; the chunks follow each other on the stream and only the first starts the records.
// The outlyingness (sd_rp_outlyingness), per chunk of directions: the rows of Z, a copy of them sorted by K10's row sort,
// K12's pd_locscale_kernel on the sorted rows, then rp_outlyingness_kernel: a thread per target takes the maximum over the
// chunk's rows of K12's o_r from the unsorted Z.  Maxima and integer sums are order-free: no result depends on the chunk.
#include "curve_routes.h"
#include "halfspace_sort.h"
#include "projection_select.h"

namespace sd {

constexpr int CP_CURVES = CV_BLOCK, CP_DIRS = 64;                   // curves and directions of a tile
constexpr int CP_TK = 16, CP_THREADS = 256, CP_R = CP_DIRS / 16, CP_C = CP_CURVES / 16;
constexpr int CP_XLD = CP_CURVES + 2, CP_ULD = CP_DIRS + 2;         // panel rows, padded (still 16-byte multiples)
constexpr i64 CP_LAUNCH_GROUPS = (i64)1 << 24;                      // workgroups of a launch at most
constexpr i64 RP_Z_VALUES = (i64)1 << 27;                           // values of Z a chunk of sd_rp_depth_sums holds (1 GiB)
constexpr int RP_THREADS = 256;

// one timepoint of the register tile: Xs and Us point at row k of the panels.  FIRST: the term starts the accumulators
template <bool FIRST>
__device__ __forceinline__ void cp_step(const double *__restrict__ Xs, const double *__restrict__ Us, int x, int y,
                                        double (&acc)[CP_R][CP_C]) {
    double a[CP_C], b[CP_R];
#pragma unroll
    for (int g = 0; g < CP_C / 2; ++g) {
        const double2 v = *reinterpret_cast<const double2 *>(Xs + 32 * g + 2 * x);
        a[2 * g] = v.x, a[2 * g + 1] = v.y;
    }
#pragma unroll
    for (int r = 0; r < CP_R; r += 2) {
        const double2 v = *reinterpret_cast<const double2 *>(Us + CP_R * y + r);
        b[r] = v.x, b[r + 1] = v.y;
    }
#pragma unroll
    for (int r = 0; r < CP_R; ++r)
#pragma unroll
        for (int c = 0; c < CP_C; ++c) {
            const double p = __dmul_rn(a[c], b[r]);
            acc[r][c] = FIRST ? p : __dadd_rn(acc[r][c], p);
        }
}

// Curves [128 (blockIdx.x % nbi) ...) x directions [r_first + 64 (blockIdx.x / nbi) ...) up to r_end.  ld: st of a time-major
// X (sn == 1), sn of a curve-major one (st == 1).  Z[(r - r_first) * n + i].
template <bool CURVE_MAJOR>
__global__ __launch_bounds__(CP_THREADS, 2) void cp_project_kernel(const double *__restrict__ X, i64 T, i64 n, i64 ld,
                                                                const double *__restrict__ U, i64 r_first, i64 r_end, i64 nbi,
                                                                double *__restrict__ Z) {
    __shared__ __attribute__((aligned(16))) double Xs[CP_TK][CP_XLD];
    __shared__ __attribute__((aligned(16))) double Us[CP_TK][CP_ULD];
    const int tid = threadIdx.x, x = tid & 15, y = tid >> 4;
    const i64 i0 = (i64)blockIdx.x % nbi * CP_CURVES, r0 = r_first + (i64)blockIdx.x / nbi * CP_DIRS;

    double acc[CP_R][CP_C];
    for (i64 t0 = 0; t0 < T; t0 += CP_TK) {
        __syncthreads();                                            // the panel before is consumed
        if constexpr (CURVE_MAJOR) {                                // lanes along t: timepoint x of the panel, curves y + 16 l
            const i64 t = t0 + x;
#pragma unroll
            for (int l = 0; l < CP_CURVES / 16; ++l) {
                const i64 i = i0 + y + 16 * l;
                Xs[x][y + 16 * l] = i < n && t < T ? X[i * ld + t] : 0.0;
            }
        } else {                                                    // lanes along the curves: rows (tid >> 7) + 2 l
            const int col = tid & (CP_CURVES - 1), k0 = tid >> 7;
            const i64 i = i0 + col;
#pragma unroll
            for (int l = 0; l < CP_TK / 2; ++l) {
                const i64 t = t0 + k0 + 2 * l;
                Xs[k0 + 2 * l][col] = i < n && t < T ? X[t * ld + i] : 0.0;
            }
        }
        {                                                           // U is row-major in t: lanes along t, directions y + 16 l
            const i64 t = t0 + x;
#pragma unroll
            for (int l = 0; l < CP_DIRS / 16; ++l) {
                const i64 r = r0 + y + 16 * l;
                Us[x][y + 16 * l] = r < r_end && t < T ? U[r * T + t] : 0.0;
            }
        }
        __syncthreads();
        const int rows = T - t0 < CP_TK ? (int)(T - t0) : CP_TK;    // the tail of the last panel is not walked
        int k = 0;
        if (t0 == 0) {
            cp_step<true>(Xs[0], Us[0], x, y, acc);
            k = 1;
        }
#pragma unroll 2
        for (; k < rows; ++k) cp_step<false>(Xs[k], Us[k], x, y, acc);
    }

#pragma unroll
    for (int r = 0; r < CP_R; ++r) {
        const i64 dir = r0 + CP_R * y + r;
        if (dir >= r_end) continue;
        double *row = Z + (dir - r_first) * n;
#pragma unroll
        for (int c = 0; c < CP_C; ++c) {
            const i64 i = i0 + 32 * (c >> 1) + 2 * x + (c & 1);
            if (i < n) row[i] = acc[r][c];
        }
    }
}

// Z[(r - r_first) * n + i] for the directions [r_first, r_end) of U and all n curves
int launch_curve_project(const double *X, i64 T, i64 n, i64 st, i64 sn, const double *U, i64 r_first, i64 r_end, double *Z,
                         hipStream_t s) {
    const i64 nbi = (n + CP_CURVES - 1) / CP_CURVES;
    i64 per = CP_LAUNCH_GROUPS / nbi;                               // direction tiles of a launch
    per = per < 1 ? 1 : per;
    const bool curve_major = sn != 1;
    for (i64 r = r_first; r < r_end; r += per * CP_DIRS) {
        const i64 left = (r_end - r + CP_DIRS - 1) / CP_DIRS;
        const dim3 grid((unsigned)(nbi * (left < per ? left : per)));
        double *Zr = Z + (r - r_first) * n;
        if (curve_major)
            hipLaunchKernelGGL((cp_project_kernel<true>), grid, dim3(CP_THREADS), 0, s, X, T, n, sn, U, r, r_end, nbi, Zr);
        else
            hipLaunchKernelGGL((cp_project_kernel<false>), grid, dim3(CP_THREADS), 0, s, X, T, n, st, U, r, r_end, nbi, Zr);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------- the depths' records
static inline size_t rp_depth_bytes(i64 rows, i64 n, int route) {
    return align_up((size_t)rows * n * 8, 256) + pair_image_plan(rows, n, route, PlanSize::of_rows(rows)).bytes;
}

RpDepthPlan rp_depth_plan(i64 n, i64 k, int route, PlanSize size) {
    i64 cap = RP_Z_VALUES / n;
    cap = cap < 1 ? 1 : cap > k ? k : cap;
    RpDepthPlan p{0, 0, 0};
    if (size.rows) {
        p.rows = size.rows < cap ? size.rows : cap;
    } else {
        if (size.bytes < rp_depth_bytes(1, n, route)) return p;
        i64 lo = 1, hi = cap;                                       // the most rows whose Z and stage 1 the bytes hold
        while (lo < hi) {
            const i64 mid = (lo + hi + 1) >> 1;
            if (rp_depth_bytes(mid, n, route) <= size.bytes) lo = mid;
            else hi = mid - 1;
        }
        p.rows = lo;
    }
    p.z = align_up((size_t)p.rows * n * 8, 256);
    p.bytes = size.rows ? rp_depth_bytes(p.rows, n, route) : size.bytes;
    return p;
}

int launch_rp_depth_sums(const double *X, i64 T, i64 n, i64 st, i64 sn, const double *U, i64 k, const i64 *targets, i64 m,
                         int route, i64 *out, void *ws, size_t ws_bytes, hipStream_t s) {
    const RpDepthPlan plan = rp_depth_plan(n, k, route, PlanSize::of_bytes(ws_bytes));
    if (!ws || plan.rows < 1) return fail(SD_ERR_WORKSPACE, "workspace below sd_rp_depth_min_workspace_bytes");
    double *Z = (double *)ws;
    for (i64 r0 = 0; r0 < k; r0 += plan.rows) {
        const i64 kk = k - r0 < plan.rows ? k - r0 : plan.rows;
        int rc = launch_curve_project(X, T, n, st, sn, U, r0, r0 + kk, Z, s);
        if (rc || (rc = launch_rank_depth_sums(Z, kk, n, targets, m, route, out, (char *)ws + plan.z, plan.bytes - plan.z, s,
                                               r0 == 0)))
            return rc;
    }
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------- the outlyingness
// a thread per target: out[j] = max(out[j], max over the chunk's rows of o_r); first: the chunk starts the maximum
__global__ __launch_bounds__(RP_THREADS) void rp_outlyingness_kernel(const double *__restrict__ Z, i64 n, int kk,
                                                                     const double *__restrict__ med,
                                                                     const double *__restrict__ mad,
                                                                     const i64 *__restrict__ targets, i64 m, int first,
                                                                     double *__restrict__ out) {
    const i64 j = (i64)blockIdx.x * RP_THREADS + threadIdx.x;
    if (j >= m) return;
    const i64 i = targets ? targets[j] : j;
    double best = first ? 0.0 : out[j];
    for (int r = 0; r < kk; ++r) {
        const double o = pd_outlyingness(Z[(i64)r * n + i], med[r], mad[r]);
        best = o > best ? o : best;
    }
    out[j] = best;
}

// fixed part (the alignment of the eight carve-outs) and the part per direction of a chunk (Z, sort buffers, med, mad)
static inline size_t rp_out_fixed() { return (size_t)(HS_SORT_CARVES + 3) * 256; }
static inline size_t rp_out_per_direction(i64 n) { return (size_t)n * 8 + hs_sort_bytes_per_direction(n) + 16; }

size_t rp_outlyingness_min_workspace_bytes(i64 n) { return rp_out_fixed() + rp_out_per_direction(n); }

size_t rp_outlyingness_workspace_bytes(i64 n, i64 k) {
    i64 kc = HS_REC_VALUES / n;
    kc = kc < 1 ? 1 : kc > k ? k : kc;
    return rp_out_fixed() + (size_t)kc * rp_out_per_direction(n);
}

int launch_rp_outlyingness(const double *X, i64 T, i64 n, i64 st, i64 sn, const double *U, i64 k, const i64 *targets, i64 m,
                           double *out, void *ws, size_t ws_bytes, hipStream_t s) {
    if (!ws || ws_bytes < rp_outlyingness_min_workspace_bytes(n))
        return fail(SD_ERR_WORKSPACE, "workspace below sd_rp_outlyingness_min_workspace_bytes");
    const i64 kc = hs_chunk_directions(ws_bytes - rp_out_fixed(), rp_out_per_direction(n), n, k);
    Carver cv(ws, ws_bytes);
    double *Z = (double *)cv.take((size_t)kc * n * 8);
    HsSortBuffers b;
    const bool carved = hs_sort_carve(cv, n, kc, b);
    double *med = (double *)cv.take((size_t)kc * 8);
    double *mad = (double *)cv.take((size_t)kc * 8);
    if (!Z || !carved || !med || !mad) return fail(SD_ERR_WORKSPACE, "workspace below sd_rp_outlyingness_min_workspace_bytes");
    for (i64 c0 = 0; c0 < k; c0 += kc) {
        const int kk = (int)(k - c0 < kc ? k - c0 : kc);
        int rc = launch_curve_project(X, T, n, st, sn, U, c0, c0 + kk, Z, s);
        if (rc) return rc;
        SD_HIP(hipMemcpyAsync(b.K[0], Z, (size_t)kk * n * 8, hipMemcpyDeviceToDevice, s));
        int src = 0;
        if ((rc = launch_hs_sort_rows(n, kk, b, &src, s)) || (rc = launch_pd_locscale(b.K[src], n, kk, med, mad, s))) return rc;
        hipLaunchKernelGGL(rp_outlyingness_kernel, dim3((unsigned)((m + RP_THREADS - 1) / RP_THREADS)), dim3(RP_THREADS), 0, s, Z,
                           n, kk, med, mad, targets, m, c0 == 0 ? 1 : 0, out);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

}  // namespace sd
