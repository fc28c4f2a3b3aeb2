// rank_routes.h -- what the translation units of the rank routes call in each other, and what the strict path calls of them
// (internal; the launchers sd_api.hip dispatches to are in sd_common.h; the strict path's own routes: strict_routes.h).  One
// declaration per signature.
#pragma once
#include "sd_common.h"
#include "strict_routes.h"

namespace sd {

constexpr u32 AB_SPECIAL = 0xFFFFFFFFu;      // u16-pair image (n <= 40 960): the curve is NaN at this timepoint

// ---- mbd_rank_bucket.hip: the bucket kernel of n <= 16 384 and its column-block form up to 40 960 ----
bool mbd_rank_bucket_supported(i64 T, i64 n, int J);
int mbd_rank_bucket_max_grid();
size_t mbd_rank_bucket_partial_bytes(i64 n, int J);
size_t mbd_rank_bucket_workspace_bytes(i64 rows, i64 n, int J);
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
bool rank_medium_supported(i64 n);
int launch_rank_medium_image(const double *Y, i64 n, i64 row0, i64 rows, u32 *AB, u32 *nnan, hipStream_t s);

// ---- mbd_rank_bucket32.hip: 32-bit key images, two workgroups per CU ----
bool rank_bucket32_supported(i64 n, i64 rows, int cus);
size_t rank_bucket32_extra_bytes(i64 rows);
int launch_rank_bucket32(const double *Y, i64 n, i64 row0, i64 rows, u32 *partial, unsigned char *rowflag, u32 *gate, u32 epoch,
                         u64 *out_zero, int G, hipStream_t s);
u32 rank_bucket32_epoch();

// ---- mbd_rank_big.hip: the B words of every (row, curve) to img[T][n], the rows' NaN counts to nnan[T] ----
int launch_rank_big_image(const double *Y, i64 T, i64 n, u32 *img, u32 *nnan, void *ws, size_t ws_bytes, hipStream_t s);

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
