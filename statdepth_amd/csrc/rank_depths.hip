// rank_depths.hip -- K14: the integrated rank depths of curves (Fraiman-Muniz, modified epigraph / hypograph index,
// modified half-region depth, integrated and infimal univariate halfspace depth).
//
// Definition.  n curves at T timepoints, time-major Y[t][i], no NaN.  For a target q at timepoint t, over the other n - 1
// curves: A = #{strictly above}, B = #{strictly below} (ties in neither).  The record of q is five int64:
//   SA = sum_t A,  SB = sum_t B,  SF = sum_t |2 A - n|,  SM = sum_t max(A, B),  MM = max_t max(A, B);
// the six depths are one fp64 expression of the record each, formed on the host (include/statdepth_hip.h, K14).
//
// Two routes write the same pairs (A, B) of every (row, curve) as a pair image and one kernel folds it:
//
// Image route (n <= 16 384), per batch of rows: launch_rank_bucket_image (mbd_rank_bucket.hip, the J >= 4 path of
//   launch_mbd_rank) writes u32[rows][n] = B | A << 16; rank_depth_fold_kernel<u32> folds it.  The batch is what the
//   workspace holds (pair_image_plan): at most 2^16 rows, at most a 1 GiB image, one row at the floor, and the
//   whole of T in one batch at the recommended size whenever T is within those caps.
//
// Sort route (any n < 2^31), per chunk of kc rows:
//   one device-to-device copy of the chunk's rows into the sort buffers;
//   launch_hs_sort_rows (halfspace.hip): K10's tile sort and merge passes with the curve's index as payload;
//   rd_rank_scatter_kernel: position p of the sorted row has lt = p and le = p + 1 unless a neighbour is equal (then a
//                        binary search finds the end of the run of ties, as in hs_rank_kernel); B = lt, A = n - le, one
//                        u64 = B | A << 32 stored at img[row][index of p].  The index is a permutation of the row: every
//                        word of the image is written once, by a plain 8-byte store.  The image takes the place of the
//                        key buffer the last merge pass read from, which is free by then;
//   rank_depth_fold_kernel<u64> folds it.  kc follows from the workspace as in K10.
//
// rank_depth_fold_kernel: block = 64 targets x 16 row slices, 8 independent loads in flight per thread (a pure stream
// over the image: the row loop of rank_fold.h, as rank_accumulate_kernel), its own LDS tree over the slices.  The first batch writes out =, later batches
// add to the four sums and take the maximum for MM.  A (target, slice) pair has one owner and the batches follow each
// other on the stream: no atomics, and integer sums and maxima do not depend on the batch size.  40 KB of LDS.
//
// The routes hand each batch's image to a RankImageConsumer (launch_rank_pair_images): the fold here, K15's transform
// into the extremity matrix in extremal.hip, K17's dominance kernel and fold in tvd.hip.  The route rule of the three and
// the plan of this stage -- rows per batch and the bytes carved for them, which the size functions and the launchers of
// all three read -- are curve_route and pair_image_plan below (curve_routes.h).
#include "curve_routes.h"
#include "rank_fold.h"
#include "halfspace_sort.h"

namespace sd {

constexpr int RD_WORDS = 5;                                        // SA, SB, SF, SM, MM
constexpr i64 RD_IMAGE_ROWS = 65536;                               // image route: rows per batch at most
constexpr size_t RD_IMAGE_BYTES = (size_t)1 << 30;                 // ... and bytes of the pair image

template <typename IMG> struct RdPair;
template <> struct RdPair<u32> {
    static __device__ __forceinline__ u32 above(u32 w) { return w >> 16; }
    static __device__ __forceinline__ u32 below(u32 w) { return w & 0xFFFFu; }
};
template <> struct RdPair<u64> {
    static __device__ __forceinline__ u32 above(u64 w) { return (u32)(w >> 32); }
    static __device__ __forceinline__ u32 below(u64 w) { return (u32)w; }
};

template <typename IMG>
__device__ __forceinline__ void rd_add(u64 (&acc)[RD_WORDS], IMG w, i64 n) {
    const u32 A = RdPair<IMG>::above(w), B = RdPair<IMG>::below(w);
    const i64 d = 2 * (i64)A - n;
    const u64 mx = A > B ? A : B;
    acc[0] += A;
    acc[1] += B;
    acc[2] += (u64)(d < 0 ? -d : d);
    acc[3] += mx;
    acc[4] = mx > acc[4] ? mx : acc[4];
}

// out[q][0 .. 5) (=, or += and max) the record of target q over the rows of one pair image
template <typename IMG>
__global__ __launch_bounds__(1024) void rank_depth_fold_kernel(const IMG *__restrict__ img, i64 rows, i64 n,
                                                               const i64 *__restrict__ targets, i64 m,
                                                               u64 *__restrict__ out, int first) {
    __shared__ u64 red[RD_WORDS][16][64];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const i64 q = (i64)blockIdx.x * 64 + x;
    const i64 i = (q < m) ? (targets ? targets[q] : q) : 0;
    u64 acc[RD_WORDS];
#pragma unroll
    for (int w = 0; w < RD_WORDS; ++w) acc[w] = 0;
    if (q < m)
        fold_rows<16, 8>(
            rows, y, [&](i64 r) { return img[r * n + i]; }, [&](IMG v, i64) { rd_add<IMG>(acc, v, n); });
#pragma unroll
    for (int w = 0; w < RD_WORDS; ++w) red[w][y][x] = acc[w];
    __syncthreads();
    if (y < RD_WORDS && q < m) {                                    // slice y finishes word y of its 64 targets
        const bool is_max = y == RD_WORDS - 1;
        u64 tot = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const u64 v = red[y][k][x];
            tot = is_max ? (v > tot ? v : tot) : tot + v;
        }
        u64 *o = out + q * RD_WORDS + y;
        if (!first) {
            const u64 old = *o;
            tot = is_max ? (old > tot ? old : tot) : old + tot;
        }
        *o = tot;
    }
}

template <typename IMG>
static int launch_rank_depth_fold(const IMG *img, i64 rows, i64 n, const i64 *targets, i64 m, u64 *out, int first,
                                  hipStream_t s) {
    hipLaunchKernelGGL((rank_depth_fold_kernel<IMG>), dim3((unsigned)((m + 63) / 64)), dim3(1024), 0, s, img, rows, n, targets, m,
                       out, first);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

// sorted rows -> img[row][column] = B | A << 32
__global__ __launch_bounds__(HS_THREADS) void rd_rank_scatter_kernel(const double *__restrict__ K, const u32 *__restrict__ I,
                                                                     i64 n, i64 total, u64 *__restrict__ img) {
    const i64 g = (i64)blockIdx.x * HS_THREADS + threadIdx.x;
    if (g >= total) return;
    const i64 r = g / n, p = g % n;
    const double *Kr = K + r * n;
    const double key = Kr[p];
    i64 lt = p, le = p + 1;
    if (p > 0 && Kr[p - 1] == key) {                                // first position of the run of ties
        i64 lo = 0, hi = p;
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if (Kr[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        lt = lo;
    }
    if (p + 1 < n && Kr[p + 1] == key) {                            // one past its last position
        i64 lo = p + 1, hi = n;
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if (Kr[mid] <= key) lo = mid + 1;
            else hi = mid;
        }
        le = lo;
    }
    const u32 col = I[g];
    if (col < n) img[r * n + col] = (u64)lt | (u64)(n - le) << 32;  // (a padding index can surface only among NaN keys)
}

// ---------------------------------------------------------------------------------------------- the plan of stage 1
int curve_route(int algo, i64 T, i64 n) {
    if (T < 1 || n < 2 || n >= ((i64)1 << 31) || algo < 0 || algo > 2) return 0;
    if (algo == 1) return n <= RD_IMAGE_MAX_N ? 1 : 0;
    return algo == 2 || n > RD_IMAGE_MAX_N ? 2 : 1;
}

static inline size_t rd_image_bytes(i64 rows, i64 n) { return align_up((size_t)rows * n * 4, 256) + align_up((size_t)rows * 4, 256); }
// What a route carves for `rows` rows.  Sort route: a fixed part (the alignment of the sort buffers' carve-outs) and a part
// per row of a chunk; the u64 image lies in the key buffer the sort has finished with.
static inline size_t rd_bytes(int route, i64 rows, i64 n) {
    return route == 1 ? rd_image_bytes(rows, n) : (size_t)HS_SORT_CARVES * 256 + (size_t)rows * hs_sort_bytes_per_direction(n);
}
// the rows the recommended size is made for: the image's caps, or K10's recommended chunk
static inline i64 rd_rows_cap(int route, i64 T, i64 n) {
    i64 r = route == 1 ? (i64)(RD_IMAGE_BYTES / ((size_t)n * 4)) : HS_REC_VALUES / n;
    r = route == 1 && r > RD_IMAGE_ROWS ? RD_IMAGE_ROWS : r;
    return r < 1 ? 1 : r > T ? T : r;
}

// A size by rows is rd_bytes of them; the rows are the most whose buffers fit the size by rd_bytes again, so a size made
// for r rows holds r of them, or more.
PairImagePlan pair_image_plan(i64 T, i64 n, int route, PlanSize size) {
    const i64 cap = rd_rows_cap(route, T, n);
    PairImagePlan p{route, 0, size.rows ? rd_bytes(route, size.rows < cap ? size.rows : cap, n) : size.bytes};
    if (p.bytes < rd_bytes(route, 1, n)) return p;
    if (route != 1) {
        p.rows = hs_chunk_directions(p.bytes - rd_bytes(route, 0, n), hs_sort_bytes_per_direction(n), n, T);
        return p;
    }
    const i64 grid_cap = (i64)device_cus() * 2048;                  // the bucket kernel's 2048 rows per workgroup of a launch
    i64 rpb = (i64)(p.bytes / ((size_t)n * 4 + 4));                 // an upper bound: rd_image_bytes(r, n) >= r (4 n + 4)
    rpb = rpb > cap ? cap : rpb;
    rpb = rpb > grid_cap ? grid_cap : rpb;
    while (rpb > 1 && rd_image_bytes(rpb, n) > p.bytes) --rpb;      // the two paddings: at most 510 bytes
    p.rows = rpb;
    return p;
}

// ---------------------------------------------------------------------------------------------- the two routes
// Each route hands the pair image of a batch (rows [row0, row0 + rows) of Y) to `use`; the image is overwritten by the next batch.
static int rank_depth_image_route(i64 rpb, const double *Y, i64 T, i64 n, RankImageConsumer &use, Carver &cv, hipStream_t s) {
    u32 *AB = (u32 *)cv.take((size_t)rpb * n * 4);
    u32 *nnan = (u32 *)cv.take((size_t)rpb * 4);
    if (!AB || !nnan) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_rank_depth_min_workspace_bytes)");
    for (i64 row0 = 0; row0 < T; row0 += rpb) {
        const i64 rows = T - row0 < rpb ? T - row0 : rpb;
        int rc = launch_rank_bucket_image(Y, n, row0, rows, AB, nnan, s);
        if (rc || (rc = use.image32(AB, row0, rows, s))) return rc;
    }
    return SD_OK;
}

static int rank_depth_sort_route(i64 kc, const double *Y, i64 T, i64 n, RankImageConsumer &use, Carver &cv, hipStream_t s) {
    HsSortBuffers b;
    if (!hs_sort_carve(cv, n, kc, b)) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_rank_depth_min_workspace_bytes)");
    for (i64 c0 = 0; c0 < T; c0 += kc) {
        const int kk = (int)(T - c0 < kc ? T - c0 : kc);
        const i64 total = (i64)kk * n;
        SD_HIP(hipMemcpyAsync(b.K[0], Y + c0 * n, (size_t)total * 8, hipMemcpyDeviceToDevice, s));
        int src = 0;
        int rc = launch_hs_sort_rows(n, kk, b, &src, s);
        if (rc) return rc;
        u64 *img = reinterpret_cast<u64 *>(b.K[src ^ 1]);          // kc x n words of 8 bytes, no longer read
        hipLaunchKernelGGL(rd_rank_scatter_kernel, dim3((unsigned)((total + HS_THREADS - 1) / HS_THREADS)), dim3(HS_THREADS), 0,
                           s, b.K[src], b.I[src], n, total, img);
        SD_HIP(hipGetLastError());
        if ((rc = use.image64(img, c0, kk, s))) return rc;
    }
    return SD_OK;
}

int launch_rank_pair_images(const PairImagePlan &plan, const double *Y, i64 T, i64 n, RankImageConsumer &use, void *ws,
                            hipStream_t s) {
    if (!ws || plan.rows < 1)
        return fail(SD_ERR_WORKSPACE, "workspace too small for one row per %s (sd_rank_depth_min_workspace_bytes)",
                    plan.route == 1 ? "batch" : "chunk");
    Carver cv(ws, plan.bytes);
    return plan.route == 1 ? rank_depth_image_route(plan.rows, Y, T, n, use, cv, s)
                           : rank_depth_sort_route(plan.rows, Y, T, n, use, cv, s);
}

// K14's consumer: the fold into the records
struct RankDepthFold final : RankImageConsumer {
    i64 n, m;
    const i64 *targets;
    u64 *out;
    bool first_rows;                                                // row 0 of Y starts the records (false: out holds earlier rows')
    RankDepthFold(i64 n_, const i64 *targets_, i64 m_, u64 *out_, bool first_rows_)
        : n(n_), m(m_), targets(targets_), out(out_), first_rows(first_rows_) {}
    int image32(const u32 *img, i64 row0, i64 rows, hipStream_t s) override {
        return launch_rank_depth_fold<u32>(img, rows, n, targets, m, out, first_rows && row0 == 0, s);
    }
    int image64(const u64 *img, i64 row0, i64 rows, hipStream_t s) override {
        return launch_rank_depth_fold<u64>(img, rows, n, targets, m, out, first_rows && row0 == 0, s);
    }
};

int launch_rank_depth_sums(const double *Y, i64 T, i64 n, const i64 *targets, i64 m, int route, i64 *out, void *ws,
                           size_t ws_bytes, hipStream_t s, bool first_rows) {
    RankDepthFold fold(n, targets, m, (u64 *)out, first_rows);
    return launch_rank_pair_images(pair_image_plan(T, n, route, PlanSize::of_bytes(ws_bytes)), Y, T, n, fold, ws, s);
}

}  // namespace sd
