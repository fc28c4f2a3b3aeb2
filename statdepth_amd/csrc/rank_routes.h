// rank_routes.h -- the route plan of a K1+K2 call, what the translation units of the rank routes call in each other, and what
// the strict path calls of them (internal; the strict path's own routes: strict_routes.h).  One declaration per signature.
#pragma once
#include "sd_common.h"
#include "strict_routes.h"

namespace sd {

constexpr u32 AB_SPECIAL = 0xFFFFFFFFu;      // u16-pair image (n <= 40 960): the curve is NaN at this timepoint

// ---- the route plan of one K1+K2 call (mbd_rank_ab.hip: mbd_plan) ----
// Every decision the size functions and the launcher take, made in one place from the shape and -- cross-check builds only --
// the SD_RANK_IMPL, SD_RANK_ROWS_PER_BATCH, SD_MEDIUM_WIDE and SD_BIG_NOMEDIUM switches (the product's xswitch() is 0).
// Computed per call: the tests change the environment between calls.
enum class MbdRoute {
    Pairwise,      // the pairwise kernel: algo says so, or auto below the thresholds
    BucketFold,    // n <= 16 384, J <= 3: the bucket kernel folds in registers, partial totals per workgroup
    PairImage,     // n <= 16 384 and J >= 4, or a retired sort generation: 16-bit pair image + fold
    MediumImage,   // 16 384 < n <= 32 768, T >= 96: column blocks through one workgroup, pair image + fold
    LargeN,        // any other n > 16 384: the chunked route (mbd_rank_big.hip)
    RetiredV1,     // SD_RANK_IMPL = 1, J <= 3: the first-generation kernel, the whole call
    None           // algo = rank for a shape no rank route covers (n = 1): SD_ERR_UNSUPPORTED
};
struct MbdPlan {
    MbdRoute route;
    int sorts;             // PairImage: 0 = the bucket kernel's image mode, else the retired generation (SD_RANK_IMPL) that ranks
    i64 rpb;               // rows of a pair image (PairImage, MediumImage)
    i64 step;              // BucketFold: rows per batch ...
    bool tl_full, tl_last; // ... and whether a batch of `step` rows / the last batch takes the two-launch path (32-bit keys)
    bool gather;           // ... into the totals of ALL curves inside the workspace; the call's subset is gathered at the end
    size_t partial_bytes;  // BucketFold: the workgroups' partial totals
    size_t ws_bytes;       // what the route's launcher gets (the caller carves it)
};
// all_targets: every curve is a target, in order (targets == NULL, tbegin == 0, m == n)
MbdPlan mbd_plan(i64 T, i64 n, i64 m, int J, int algo, bool all_targets);
// what sd_mbd_workspace_bytes reserves for algo = rank and auto: the sum over the rank routes of the shape (see there)
size_t mbd_rank_routes_workspace_bytes(i64 T, i64 n, int J);
// runs plan.route (any but Pairwise) with plan.ws_bytes at ws
int launch_mbd_rank(const MbdPlan &plan, const double *Y, i64 T, i64 n, const i64 *targets, i64 tbegin, i64 m, int J, u64 *out,
                    void *ws, hipStream_t s);

// ---- mbd_rank_bucket.hip: the bucket kernel of n <= 16 384 ----
// the kernel's `p32` argument: how a workgroup's partial totals travel (J = 2 only above 0)
enum : int {
    RB_PARTIAL_U64 = 0,    // u64 blocks
    RB_PARTIAL_U32 = 1,    // u32 blocks: ceil(rows / G) * C(n-1, 2) < 2^32
    RB_PARTIAL_ACC32 = 2   // ... and 32-bit accumulators in the kernel: ceil(rows / G) * n^2 < 2^32
};
size_t mbd_rank_bucket_partial_bytes(i64 n, int J);
int launch_rank_bucket(const double *Y, i64 n, i64 row0, i64 rows, int J, u64 *partial, int *p32_out, int *G_out,
                       hipStream_t s);
int launch_rank_bucket_image(const double *Y, i64 n, i64 row0, i64 rows, u32 *AB, u32 *nnan, hipStream_t s);
bool rank_bucket_two_level_supported(i64 n, i64 rows);
int launch_rank_bucket_two_level(const double *Y, i64 n, i64 row0, i64 rows, u64 *partial, u64 *out, int first, hipStream_t s);
u64 *rank_bucket_two_level_all_totals(u64 *partial, i64 n);
int launch_rank_gather_totals(const u64 *all, const i64 *targets, i64 tbegin, i64 m, u64 *out, hipStream_t s);
int launch_rank_finalize(const u64 *partial, int G, int p32, const u32 *AB, const u32 *nnan, const unsigned char *rowflag,
                         i64 rows, i64 n, const i64 *targets, i64 tbegin, i64 m, int J, u64 *out, int first,
                         hipStream_t s);

// ---- mbd_rank_medium.hip: the bucket structure over 2 or 3 column blocks, 16 384 < n <= 40 960 (the external targets'
// kernel, mbd_rank_external.hip, shares its row build -- rank_bucket_row.h; its entry points: sd_common.h) ----
bool rank_medium_supported(i64 n);
int launch_rank_medium_image(const double *Y, i64 n, i64 row0, i64 rows, u32 *AB, u32 *nnan, hipStream_t s);

// ---- mbd_rank_bucket32.hip: 32-bit key images, two workgroups per CU ----
bool rank_bucket32_supported(i64 n, i64 rows, int cus);
size_t rank_bucket32_extra_bytes(i64 rows);
int launch_rank_bucket32(const double *Y, i64 n, i64 row0, i64 rows, u32 *partial, unsigned char *rowflag, u32 *gate, u32 epoch,
                         u64 *out_zero, int G, hipStream_t s);
u32 rank_bucket32_epoch();

// ---- mbd_rank_big.hip: the large-n route; its image form: the B words of every (row, curve) to img[T][n], the rows' NaN
// counts to nnan[T] (mbd_rank_big_supported, mbd_rank_big_workspace_bytes: sd_common.h, the strict path sizes by them) ----
int launch_mbd_rank_big(const double *Y, i64 T, i64 n, const i64 *targets, i64 tbegin, i64 m, int J,
                        u64 *out, void *ws, size_t ws_bytes, hipStream_t s);
int launch_rank_big_image(const double *Y, i64 T, i64 n, u32 *img, u32 *nnan, void *ws, size_t ws_bytes, hipStream_t s);

// ---- mbd_rank_fold.hip: out (=|+=, first) the band counts of the targets over the rows of one pair image: the 16-bit image
// B | A << 16 of the routes above, the AB2 image of the large-n route (rank_big_common.h; skeleton: rank_fold.h) ----
struct AB2;
int fold_pair_image(const u32 *AB, const u32 *nnan, i64 rows, i64 n, const i64 *targets, i64 tbegin, i64 m, int J, u64 *out,
                    int first, hipStream_t s);
int fold_ab2_image(const AB2 &ab, const u32 *nnan, i64 rows, i64 n, const i64 *targets, i64 tbegin, i64 m, int J, u64 *out,
                   int first, hipStream_t s);

// ---- the retired generations, one hook per point where a cross-check switch diverts a product route ----
// libstatdepth_hip_xcheck.so: defined next to the retired kernels (mbd_rank_ab_retired.hip, mbd_rank.hip,
// mbd_rank_big_retired.hip).  The product library: xcheck.hip defines them to fail with SD_ERR_UNSUPPORTED; nothing
// calls them there, because xswitch() is 0.
// SD_RANK_IMPL = 3, 2: the sort kernels write the pair image of rows [row0, row0 + rows)
int retired_rank_sorts(const double *Y, i64 n, i64 row0, i64 rows, u32 *AB, u32 *nnan, int impl, hipStream_t s);
// SD_RANK_IMPL = 1 (J <= 3): the first-generation rank kernel, the whole call
int retired_rank_v1(const double *Y, i64 T, i64 n, const i64 *targets, i64 tbegin, i64 m, int J, u64 *out, void *ws,
                    size_t ws_bytes, hipStream_t s);
// SD_BIG_GEN2 / SD_BIG_SORT / SD_BIG_PART1 / SD_BIG_IMPL = 1: one batch of the large-n route (BigBatch: rank_big_common.h)
struct BigBatch;
int retired_big_rank_batch(const BigBatch &b, hipStream_t s, const u32 **nnan_rows);

}  // namespace sd
