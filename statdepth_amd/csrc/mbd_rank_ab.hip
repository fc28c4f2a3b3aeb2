// mbd_rank_ab.hip -- K1+K2 rank formulation: the route plan (mbd_plan) and the launcher of the rank path.
//
// Same integers as the pairwise kernel and the reference's enumeration (_functional.py:246-251,
// _containment.py:75-77): per (curve, timepoint) the counts B (others strictly below) and A (strictly above), and
// C(v,j) - C(A,j) - C(B,j) summed over t.
//
// The rows are ranked by rank_bucket_kernel (mbd_rank_bucket.hip): J <= 3 folds in registers,
// J >= 4 writes the pairs (B, A) of every (row, curve) as a uint16 pair image and
//  C  fold_pair_image (mbd_rank_fold.hip: rank_accumulate_kernel / rank_accumulate4_kernel) folds the pairs and the
//     per-row NaN counts into the int64 totals of the requested targets.
// The sort-based predecessors the bucket kernel replaced live in mbd_rank_ab_retired.hip and mbd_rank.hip (cross-check
// library only) and are reached through retired_rank_sorts / retired_rank_v1 (rank_routes.h) when SD_RANK_IMPL asks.

#include "sd_common.h"
#include "rank_routes.h"

namespace sd {

// ---------------------------------------------------------------------------------------------------
// the route plan (rank_routes.h): which route takes a shape, its batches and its workspace
// ---------------------------------------------------------------------------------------------------
static i64 image_rows_per_batch(i64 T, i64 n) {
    i64 r = ((i64)1 << 30) / (n * 4);       // pair image <= 1 GiB
    if (r > 65536) r = 65536;               // and the bucket kernel's per-workgroup bitmap of set-aside rows (2048 bits)
    const i64 v = xswitch("SD_RANK_ROWS_PER_BATCH");   // cross-check builds: force several batches on small inputs
    if (v > 0 && v < r) r = v;
    if (r < 1) r = 1;
    return r < T ? r : T;
}

MbdPlan mbd_plan(i64 T, i64 n, i64 m, int J, int algo, bool all_targets) {
    MbdPlan p{};
    p.route = MbdRoute::Pairwise;
    const bool jok = J >= 2 && J <= JMAX;
    const bool small = jok && n >= 2 && n <= 16384, large = mbd_rank_big_supported(T, n, J);
    // auto: rank costs ~n log n per timepoint whatever m is, pairwise costs m*n; the chunked rank of n > 16 384 costs
    // ~(n/C) sorts + (n/C)^2 searches per row whatever m is
    if (algo == SD_MBD_PAIRWISE || (algo != SD_MBD_RANK && !(small && m >= 32) && !(large && m >= 2048))) return p;
    // 16 384 < n <= 32 768: pair image by rank_medium_image_kernel (2 column blocks per workgroup).  One workgroup per row: with
    // fewer than 96 rows the large-n route, which spreads a row over several workgroups, fills the chip better
    // ... and since the large-n route's third generation (round 3) three column blocks lose to it: 40 960 x 500 in 0.322 against
    // 0.287 ms, 32 768 (two blocks) 0.263 against 0.267.  Cross-check builds, SD_MEDIUM_WIDE = 1: up to the kernel's 40 960
    const i64 top = xswitch("SD_MEDIUM_WIDE") == 1 ? (i64)40960 : (i64)32768;
    if (jok && rank_medium_supported(n) && n <= top && T >= 96 && xswitch("SD_BIG_NOMEDIUM") != 1) {
        p.route = MbdRoute::MediumImage;
        p.rpb = image_rows_per_batch(T, n);
        p.ws_bytes = align_up((size_t)p.rpb * n * 4, 256) + align_up((size_t)p.rpb * 4, 256) + 512;
    } else if (large) {
        p.route = MbdRoute::LargeN;
        p.ws_bytes = mbd_rank_big_workspace_bytes(T, n, J);
    } else if (!small) {
        p.route = MbdRoute::None;
    } else {
        // the bucket kernel ranks the rows: folding in registers (J <= 3) or writing the pair image (J >= 4).  In the cross-check
        // library SD_RANK_IMPL selects the image mode (5) and the sort-based predecessors 3, 2, 1.
        const int forced = (int)xswitch("SD_RANK_IMPL");
        const int impl = forced == 0 || (forced == 4 && J >= 4) ? (J <= 3 ? 4 : 5) : forced;
        p.rpb = image_rows_per_batch(T, n);
        if (impl == 4) {
            p.route = MbdRoute::BucketFold;                 // measured faster than the sort kernels from n = 600 to 16384
            p.partial_bytes = mbd_rank_bucket_partial_bytes(n, J);
            p.ws_bytes = p.partial_bytes + 512;             // no pair image on this route
            // the two-launch path takes up to 4 096 rows per batch (its list of flagged rows sits in LDS): longer series go
            // through it in batches of that size, the last one through whichever path takes its length
            p.step = (J == 2 && p.rpb > 4096 && rank_bucket_two_level_supported(n, 4096)) ? 4096 : p.rpb;
            if (J == 2) {
                const i64 last = T - (T - 1) / p.step * p.step;                       // rows of the last batch
                const bool full = T > last && rank_bucket_two_level_supported(n, p.step), end = rank_bucket_two_level_supported(n, last);
                // a call for a subset of the targets ranks every row all the same: the path computes the totals of ALL curves
                // into the workspace and the subset is gathered at the end -- provided every batch of the call takes this path
                p.gather = !all_targets && (full || T == last) && end && m >= 1;
                p.tl_full = (all_targets || p.gather) && full;
                p.tl_last = (all_targets || p.gather) && end;
            }
        } else {
            p.route = (impl == 1 && J <= 3) ? MbdRoute::RetiredV1 : MbdRoute::PairImage;
            p.sorts = impl == 5 ? 0 : impl;
            // (the sizes are the ones this route always had: a second row array, and the first generation's partial sums)
            const size_t need = align_up((size_t)p.rpb * n * 4, 256) + 2 * align_up((size_t)p.rpb * 4, 256) + 512;
            const size_t v1 = (size_t)(T < 1024 ? T : 1024) * (J <= 3 ? J - 1 : 0) * n * 8;
            p.ws_bytes = need > v1 ? need : v1;
        }
    }
    return p;
}

size_t mbd_rank_routes_workspace_bytes(i64 T, i64 n, int J) {
    const MbdPlan p = mbd_plan(T, n, n, J, SD_MBD_RANK, true);
    return p.ws_bytes + (p.route == MbdRoute::MediumImage ? mbd_rank_big_workspace_bytes(T, n, J) : 0);
}

int launch_mbd_rank(const MbdPlan &plan, const double *Y, i64 T, i64 n, const i64 *targets, i64 tbegin, i64 m, int J, u64 *out,
                    void *ws, hipStream_t s) {
    switch (plan.route) {
        case MbdRoute::LargeN: return launch_mbd_rank_big(Y, T, n, targets, tbegin, m, J, out, ws, plan.ws_bytes, s);
        case MbdRoute::RetiredV1: return retired_rank_v1(Y, T, n, targets, tbegin, m, J, out, ws, plan.ws_bytes, s);
        case MbdRoute::BucketFold: case MbdRoute::PairImage: case MbdRoute::MediumImage: break;
        default: return fail(SD_ERR_UNSUPPORTED, "rank kernel does not cover T=%lld n=%lld J=%d", (long long)T, (long long)n, J);
    }
    Carver cv(ws, plan.ws_bytes);
    int rc;
    if (plan.route == MbdRoute::BucketFold) {
        // the bucket kernel ranks every row itself: partial totals per workgroup, no pair image, no search launch
        u64 *partial = (u64 *)cv.take(plan.partial_bytes);
        if (!partial) return fail(SD_ERR_WORKSPACE, "rank workspace too small (bucket kernel)");
        u64 *const tl_out = plan.gather ? rank_bucket_two_level_all_totals(partial, n) : out;
        for (i64 row0 = 0; row0 < T; row0 += plan.step) {
            const i64 rows = T - row0 < plan.step ? T - row0 : plan.step;
            int G = 0, p32 = RB_PARTIAL_U64;
            if (row0 + plan.step < T ? plan.tl_full : plan.tl_last) {
                // 32-bit key images, two workgroups per CU; the second launch finalizes (and ranks what the first flagged)
                if ((rc = launch_rank_bucket_two_level(Y, n, row0, rows, partial, tl_out, row0 == 0, s))) return rc;
                continue;
            }
            if ((rc = launch_rank_bucket(Y, n, row0, rows, J, partial, &p32, &G, s))) return rc;
            if ((rc = launch_rank_finalize(partial, G, p32, nullptr, nullptr, nullptr, rows, n, targets, tbegin, m, J, out,
                                           row0 == 0, s)))
                return rc;
        }
        return plan.gather ? launch_rank_gather_totals(tl_out, targets, tbegin, m, out, s) : SD_OK;
    }
    // pair image: the bucket kernel's image mode, its column-block form, or the sort kernels of a cross-check build
    u32 *AB = (u32 *)cv.take((size_t)plan.rpb * n * 4);
    u32 *nnan = (u32 *)cv.take((size_t)plan.rpb * 4);
    if (!AB || !nnan) return fail(SD_ERR_WORKSPACE, "rank workspace too small");
    for (i64 row0 = 0; row0 < T; row0 += plan.rpb) {
        const i64 rows = T - row0 < plan.rpb ? T - row0 : plan.rpb;
        rc = plan.route == MbdRoute::MediumImage ? launch_rank_medium_image(Y, n, row0, rows, AB, nnan, s)
             : plan.sorts                       ? retired_rank_sorts(Y, n, row0, rows, AB, nnan, plan.sorts, s)
                                                : launch_rank_bucket_image(Y, n, row0, rows, AB, nnan, s);
        if (rc || (rc = fold_pair_image(AB, nnan, rows, n, targets, tbegin, m, J, out, row0 == 0, s))) return rc;
    }
    return SD_OK;
}

}  // namespace sd

