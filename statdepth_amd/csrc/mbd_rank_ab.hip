// mbd_rank_ab.hip -- K1+K2 rank formulation for n <= 16384: the launcher of the rank path and the kernels that fold a
// pair image.
//
// Same integers as the pairwise kernel and the reference's enumeration (_functional.py:246-251,
// _containment.py:75-77): per (curve, timepoint) the counts B (others strictly below) and A (strictly above), and
// C(v,j) - C(A,j) - C(B,j) summed over t.
//
// The rows are ranked by rank_bucket_kernel (mbd_rank_bucket.hip): J <= 3 folds in registers,
// J >= 4 writes the pairs (B, A) of every (row, curve) as a uint16 pair image and
//  C  rank_accumulate_kernel / rank_accumulate4_kernel -- fold the pairs and the per-row NaN counts into the int64
//     totals of the requested targets.
// The sort-based predecessors the bucket kernel replaced live in mbd_rank_ab_retired.hip and mbd_rank.hip (cross-check
// library only) and are reached through retired_rank_sorts / retired_rank_v1 (rank_routes.h) when SD_RANK_IMPL asks.

#include "sd_common.h"
#include "rank_routes.h"

namespace sd {

// ---------------------------------------------------------------------------------------------------
// C: out[q][j] += sum over the batch's rows of the band counts of target q.
// block = 64 targets x 16 row slices, LDS tree over the slices.
// ---------------------------------------------------------------------------------------------------
template <int J>
__global__ __launch_bounds__(1024) void rank_accumulate_kernel(const u32 *__restrict__ AB, const u32 *__restrict__ nnan,
                                                               i64 rows, i64 n, const i64 *__restrict__ targets,
                                                               i64 tbegin, i64 m, u64 *__restrict__ out, int first) {
    __shared__ u64 red[16][64];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const i64 q = (i64)blockIdx.x * 64 + x;
    const i64 i = (q < m) ? (targets ? targets[q] : tbegin + q) : 0;
    u64 acc[JMAX - 1];
#pragma unroll
    for (int j = 0; j < JMAX - 1; ++j) acc[j] = 0;
    if (q < m) {
        // 8 independent loads in flight per thread: this kernel is a pure stream over the pair image
        i64 r = y;
        for (; r + 16 * 7 < rows; r += 16 * 8) {
            u32 ab[8], nn[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                ab[u] = AB[(r + 16 * u) * n + i];
                nn[u] = nnan[r + 16 * u];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (ab[u] != AB_SPECIAL) band_counts_add<J>(ab[u] >> 16, ab[u] & 0xFFFFu, nn[u], (u64)(n - 1), acc);
        }
        for (; r < rows; r += 16) {
            const u32 ab = AB[r * n + i];
            if (ab != AB_SPECIAL) band_counts_add<J>(ab >> 16, ab & 0xFFFFu, nnan[r], (u64)(n - 1), acc);
        }
    }
#pragma unroll
    for (int j = 0; j < J - 1; ++j) {
        red[y][x] = acc[j];
        __syncthreads();
        if (y == 0 && q < m) {
            u64 tot = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) tot += red[k][x];
            if (first) out[q * (J - 1) + j] = tot;
            else out[q * (J - 1) + j] += tot;
        }
        __syncthreads();
    }
}

// Same fold for a contiguous, 4-aligned target block: 16-byte loads (4 curves per lane, 1 KiB per wave
// instruction instead of 256 B).  block = 16 curve quads x 64 row slices.
template <int J>
__global__ __launch_bounds__(1024) void rank_accumulate4_kernel(const u32 *__restrict__ AB, const u32 *__restrict__ nnan,
                                                                i64 rows, i64 n, i64 tbegin, i64 m,
                                                                u64 *__restrict__ out, int first) {
    __shared__ u64 red[64][65];
    const int x = threadIdx.x & 15, y = threadIdx.x >> 4;            // quad within block, row slice
    const i64 q4 = ((i64)blockIdx.x * 16 + x) * 4;                   // first of this thread's 4 targets
    const bool live = q4 < m;
    u64 acc[4][JMAX - 1];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < JMAX - 1; ++j) acc[c][j] = 0;
    if (live) {
        const u32 *src = AB + tbegin + q4;
        i64 r = y;
        for (; r + 64 * 3 < rows; r += 64 * 4) {
            uint4 v[4];
            u32 nn[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = *reinterpret_cast<const uint4 *>(src + (r + 64 * u) * n);
                nn[u] = nnan[r + 64 * u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const u32 ab[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (ab[c] != AB_SPECIAL) band_counts_add<J>(ab[c] >> 16, ab[c] & 0xFFFFu, nn[u], (u64)(n - 1), acc[c]);
            }
        }
        for (; r < rows; r += 64) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + r * n);
            const u32 nn = nnan[r];
            const u32 ab[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (ab[c] != AB_SPECIAL) band_counts_add<J>(ab[c] >> 16, ab[c] & 0xFFFFu, nn, (u64)(n - 1), acc[c]);
        }
    }
#pragma unroll
    for (int j = 0; j < J - 1; ++j) {
#pragma unroll
        for (int c = 0; c < 4; ++c) red[y][x * 4 + c] = acc[c][j];
        __syncthreads();
        if (threadIdx.x < 64) {
            const i64 q = (i64)blockIdx.x * 64 + threadIdx.x;
            if (q < m) {
                u64 tot = 0;
                for (int k = 0; k < 64; ++k) tot += red[k][threadIdx.x];
                if (first) out[q * (J - 1) + j] = tot;
                else out[q * (J - 1) + j] += tot;
            }
        }
        __syncthreads();
    }
}

static i64 ab_rows_per_batch(i64 T, i64 n) {
    i64 r = ((i64)1 << 30) / (n * 4);       // pair image <= 1 GiB
    if (r > 65536) r = 65536;               // and the bucket kernel's per-workgroup bitmap of set-aside rows (2048 bits)
    const i64 v = xswitch("SD_RANK_ROWS_PER_BATCH");   // cross-check builds: force several batches on small inputs
    if (v > 0 && v < r) r = v;
    if (r < 1) r = 1;
    return r < T ? r : T;
}

bool mbd_rank_supported(i64 T, i64 n, int J) {
    (void)T;
    return n >= 2 && n <= 16384 && J >= 2 && J <= JMAX;
}

// Which implementation ranks the rows: 4 = bucket kernel (J <= 3), 5 = bucket kernel in pair-image mode +
// fold (J >= 4).  In the cross-check library SD_RANK_IMPL selects the sort-based predecessors 3, 2, 1.
static int rank_impl(i64 T, i64 n, int J) {
    const int forced = (int)xswitch("SD_RANK_IMPL");
    int impl = forced ? forced : 4;
    if (impl == 4 && !mbd_rank_bucket_supported(T, n, J)) impl = (J >= 4) ? 5 : 3;
    return impl;
}

size_t mbd_rank_workspace_bytes(i64 T, i64 n, int J) {
    if (!mbd_rank_supported(T, n, J)) return 0;
    const i64 rpb = ab_rows_per_batch(T, n);
    const int impl = rank_impl(T, n, J);
    if (impl == 4) return mbd_rank_bucket_workspace_bytes(rpb, n, J);      // no pair image on this path
    size_t need = align_up((size_t)rpb * n * 4, 256) + 2 * align_up((size_t)rpb * 4, 256) + 512;
    size_t v1 = (size_t)(T < 1024 ? T : 1024) * (J <= 3 ? J - 1 : 0) * n * 8;   // first-generation kernel's partial sums
    return need > v1 ? need : v1;
}

// out (=|+=, first) the band counts of the targets over the rows of one pair image
static int fold_pair_image(const u32 *AB, const u32 *nnan, i64 rows, i64 n, const i64 *targets, i64 tbegin, i64 m, int J,
                           u64 *out, int first, hipStream_t s) {
    dim3 grid((unsigned)((m + 63) / 64));
    if (!targets && (n % 4) == 0 && (tbegin % 4) == 0 && (m % 4) == 0 && J <= 3) {
        SD_DISPATCH_J(J, hipLaunchKernelGGL((rank_accumulate4_kernel<J_>), grid, dim3(1024), 0, s, AB, nnan, rows, n, tbegin, m,
                                            out, first));
    } else {
        SD_DISPATCH_J(J, hipLaunchKernelGGL((rank_accumulate_kernel<J_>), grid, dim3(1024), 0, s, AB, nnan, rows, n, targets,
                                            tbegin, m, out, first));
    }
    SD_HIP(hipGetLastError());
    return SD_OK;
}

int launch_mbd_rank(const double *Y, i64 T, i64 n, const i64 *targets, i64 tbegin, i64 m, int J,
                    u64 *out, void *ws, size_t ws_bytes, hipStream_t s) {
    if (!mbd_rank_supported(T, n, J)) return fail(SD_ERR_UNSUPPORTED, "rank kernels cover 2 <= n <= 16384");
    const int impl = rank_impl(T, n, J);
    if (impl == 1 && J <= 3) return retired_rank_v1(Y, T, n, targets, tbegin, m, J, out, ws, ws_bytes, s);
    const i64 rpb = ab_rows_per_batch(T, n);
    Carver cv(ws, ws_bytes);
    if (impl == 4) {
        // the bucket kernel ranks every row itself: partial totals per workgroup, no pair image, no search launch
        u64 *partial = (u64 *)cv.take(mbd_rank_bucket_partial_bytes(n, J));
        if (!partial) return fail(SD_ERR_WORKSPACE, "rank workspace too small (bucket kernel)");
        // the two-launch path takes up to 4 096 rows per batch (its list of flagged rows sits in LDS): longer series go
        // through it in batches of that size, the last one through whichever path takes its length
        // (a call for a subset of the targets ranks every row all the same: the path computes the totals of ALL curves into
        // the workspace and the subset is gathered at the end -- provided every batch of the call takes this path)
        const bool all_targets = !targets && tbegin == 0 && m == n;
        const i64 step = (J == 2 && rpb > 4096 && rank_bucket_two_level_supported(n, 4096)) ? 4096 : rpb;
        bool every = J == 2;                                            // does every batch of this call take the two-launch path?
        for (i64 row0 = 0; row0 < T && every; row0 += step) every = rank_bucket_two_level_supported(n, T - row0 < step ? T - row0 : step);
        const bool subset_tl = !all_targets && every && m >= 1;
        const bool two_level = J == 2 && (all_targets || subset_tl);
        u64 *const tl_out = subset_tl ? rank_bucket_two_level_all_totals(partial, n) : out;
        for (i64 row0 = 0; row0 < T; row0 += step) {
            const i64 rows = T - row0 < step ? T - row0 : step;
            int rc, G = 0, p32 = 0;
            if (two_level && rank_bucket_two_level_supported(n, rows)) {
                // 32-bit key images, two workgroups per CU; the second launch finalizes (and ranks what the first flagged)
                if ((rc = launch_rank_bucket_two_level(Y, n, row0, rows, partial, tl_out, row0 == 0, s))) return rc;
                continue;
            }
            if ((rc = launch_rank_bucket(Y, n, row0, rows, J, partial, &p32, &G, s))) return rc;
            if ((rc = launch_rank_finalize(partial, G, p32, nullptr, nullptr, nullptr, rows, n, targets, tbegin, m, J, out,
                                           row0 == 0, s)))
                return rc;
        }
        if (tl_out != out) return launch_rank_gather_totals(tl_out, targets, tbegin, m, out, s);
        return SD_OK;
    }
    // pair image: the bucket kernel's image mode (5), or the sort kernels of a cross-check build (3, 2, 1)
    u32 *AB = (u32 *)cv.take((size_t)rpb * n * 4);
    u32 *nnan = (u32 *)cv.take((size_t)rpb * 4);
    if (!AB || !nnan) return fail(SD_ERR_WORKSPACE, "rank workspace too small");
    for (i64 row0 = 0; row0 < T; row0 += rpb) {
        const i64 rows = T - row0 < rpb ? T - row0 : rpb;
        int rc = impl == 5 ? launch_rank_bucket_image(Y, n, row0, rows, AB, nnan, s)
                           : retired_rank_sorts(Y, n, row0, rows, AB, nnan, impl, s);
        if (rc || (rc = fold_pair_image(AB, nnan, rows, n, targets, tbegin, m, J, out, row0 == 0, s))) return rc;
    }
    return SD_OK;
}

// 16 384 < n <= 40 960: pair image by rank_medium_image_kernel (2 or 3 column blocks per workgroup, mbd_rank_bucket.hip),
// folded by the same accumulate kernels as the bucket kernel's image mode.
bool mbd_rank_medium_supported(i64 T, i64 n, int J) {
    // one workgroup per row: with few rows the large-n route, which spreads a row over several workgroups, fills the chip better
    // ... and since the large-n route's third generation (round 3) three column blocks lose to it: 40 960 x 500 in 0.322 against
    // 0.287 ms, 32 768 (two blocks) 0.263 against 0.267.  Cross-check builds, SD_MEDIUM_WIDE = 1: up to the kernel's 40 960
    const i64 top = xswitch("SD_MEDIUM_WIDE") == 1 ? (i64)40960 : (i64)32768;
    return rank_medium_supported(n) && n <= top && T >= 96 && J >= 2 && J <= JMAX && xswitch("SD_BIG_NOMEDIUM") != 1;
}

size_t mbd_rank_medium_workspace_bytes(i64 T, i64 n, int J) {
    if (!mbd_rank_medium_supported(T, n, J)) return 0;
    const i64 rpb = ab_rows_per_batch(T, n);
    return align_up((size_t)rpb * n * 4, 256) + align_up((size_t)rpb * 4, 256) + 512;
}

int launch_mbd_rank_medium(const double *Y, i64 T, i64 n, const i64 *targets, i64 tbegin, i64 m, int J, u64 *out, void *ws,
                           size_t ws_bytes, hipStream_t s) {
    if (!mbd_rank_medium_supported(T, n, J)) return fail(SD_ERR_UNSUPPORTED, "medium rank route covers 16384 < n <= 32768 with T >= 96");
    const i64 rpb = ab_rows_per_batch(T, n);
    Carver cv(ws, ws_bytes);
    u32 *AB = (u32 *)cv.take((size_t)rpb * n * 4);
    u32 *nnan = (u32 *)cv.take((size_t)rpb * 4);
    if (!AB || !nnan) return fail(SD_ERR_WORKSPACE, "rank workspace too small (medium route)");
    for (i64 row0 = 0; row0 < T; row0 += rpb) {
        const i64 rows = T - row0 < rpb ? T - row0 : rpb;
        int rc = launch_rank_medium_image(Y, n, row0, rows, AB, nnan, s);
        if (rc || (rc = fold_pair_image(AB, nnan, rows, n, targets, tbegin, m, J, out, row0 == 0, s))) return rc;
    }
    return SD_OK;
}

}  // namespace sd
