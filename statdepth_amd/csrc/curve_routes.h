// curve_routes.h -- the curve depths on K14's pair image (K14 rank depths, K15 extremal depth, K17 total variation depth):
// their one route rule, the plan of stage 1 that the size functions and the launchers read, and each family's own plan
// built on it; and the metric depths, which read the doubles: K20, the squared L2 distances of curves, K21, the functional
// spatial depth on them, and K22, the lune depths on their matrix -- their one target selector, their one plan over blocks of
// targets and the two walks of their launchers (internal; the K1+K2 rank routes: rank_routes.h, the strict path's:
// strict_routes.h).
#pragma once
#include "sd_common.h"

namespace sd {

constexpr i64 RD_IMAGE_MAX_N = 16384;                               // curves of a row the bucket kernel's image holds

// The route of a call (rank_depths.hip): 1 = the u32 pair image of the bucket kernel (K14, K15: "image", K17: "LDS";
// n <= RD_IMAGE_MAX_N), 2 = K10's sort and a u64 pair image (K14, K15: "sort") or K17's pairwise kernel, any n < 2^31;
// 0 where the shape (T < 1, n < 2, n >= 2^31) or the algo (0 auto, 1, 2) has none.
int curve_route(int algo, i64 T, i64 n);

// What a plan is sized by: the bytes at hand behind the time-major copy, or a number of rows per batch -- all T for the
// recommended size, which the route's caps cut down, one row for the floor.
struct PlanSize {
    size_t bytes;
    i64 rows;                                                       // 0: by bytes
    static PlanSize of_bytes(size_t b) { return {b, 0}; }
    static PlanSize of_rows(i64 r) { return {0, r}; }
};

// ---- stage 1 (rank_depths.hip): the pair image of Y, batch by batch ----
struct PairImagePlan {
    int route;
    i64 rows;                                                       // per batch (route 1) or per chunk (route 2); 0: below the floor
    size_t bytes;                                                   // what stage 1 carves for them
};
// By bytes: the most rows they hold within the route's caps.  By rows: the size for them, and the rows that size holds
// -- more than asked for where the 256-byte padding of a small image leaves room (32 rows at n = 2).
PairImagePlan pair_image_plan(i64 T, i64 n, int route, PlanSize size);

// What takes the pair image of one batch of rows [row0, row0 + rows) of Y, img[r][i] of row row0 + r and curve i: B | A << 16
// in u32 on route 1, B | A << 32 in u64 on route 2.  It enqueues on s; the next batch overwrites the image.
struct RankImageConsumer {
    virtual int image32(const u32 *img, i64 row0, i64 rows, hipStream_t s) = 0;
    virtual int image64(const u64 *img, i64 row0, i64 rows, hipStream_t s) = 0;
    virtual ~RankImageConsumer() = default;
};
// runs plan.route in batches of plan.rows rows, with plan.bytes at ws
int launch_rank_pair_images(const PairImagePlan &plan, const double *Y, i64 T, i64 n, RankImageConsumer &use, void *ws,
                            hipStream_t s);

// ---- K14 integrated rank depths of curves (rank_depths.hip): out[q] = (SA, SB, SF, SM, MM).  Its plan is stage 1's. ----
// first_rows: Y holds the first rows of the matrix, so its first batch starts the records; false where the caller feeds the
// rows in chunks (K23) and this chunk adds to what the chunks before it left in out.
int launch_rank_depth_sums(const double *Y, i64 T, i64 n, const i64 *targets, i64 m, int route, i64 *out, void *ws,
                           size_t ws_bytes, hipStream_t s, bool first_rows = true);

// ---- K15 extremal depth of curves (extremal.hip): out[q] = #{curves i : v_i >=lex v_q}, v the descending sort of |A - B|
// over time.  The extremity matrix E and the heads H, then stage 1. ----
constexpr i64 EX_MAX_T = 16384;                                     // keys one sort workgroup holds in LDS (64 KiB): the caller checks
struct ExtremalPlan {
    PairImagePlan stage1;
    size_t bytes;                                                   // E, H and stage 1
};
ExtremalPlan extremal_plan(i64 T, i64 n, int route, PlanSize size);
int launch_extremal_counts(const double *Y, i64 T, i64 n, const i64 *targets, i64 m, int route, i64 *out, void *ws,
                           size_t ws_bytes, hipStream_t s);

// ---- K17 total variation depth and shape similarity of curves (tvd.hip): sd_sum[q] = SD, shape[q] = (SS, SN, SW), counts
// (null or [T - 1][m]) = c_t.  The slices' records; on route 1 then the carried row, C for stage1.rows rows and stage 1. ----
struct TvdPlan {
    PairImagePlan stage1;                                           // route 1
    i64 rows;                                                       // per batch: stage1.rows, or all T on route 2; 0: below the floor
    size_t bytes;                                                   // the whole of it
};
TvdPlan tvd_plan(i64 T, i64 n, i64 m, int route, PlanSize size);
int launch_tvd_sums(const double *Y, i64 T, i64 n, const i64 *targets, i64 m, int route, i64 *sd_sum, double *shape,
                    u32 *counts, void *ws, size_t ws_bytes, hipStream_t s);

// ---- The metric depths of curves: K20, K21 and K22 read the doubles, not the pair image.  What they share: ----
// The targets of a call: sample curves (targets null: all in order, m == n) or the m columns of Q (T x m, time-major dense).  The
// kernels take the panel as plain arguments and read the value (t, q) at P[t * ldp + (targets ? targets[q] : q)].
struct CurveSel {
    const double *Q;
    const i64 *targets;
    const double *panel(const double *Y) const { return Q ? Q : Y; }   // P
    i64 ld(i64 n, i64 m) const { return Q ? m : n; }                    // ldp
};
static inline CurveSel select_sample(const i64 *targets) { return CurveSel{nullptr, targets}; }
static inline CurveSel select_columns(const double *Q) { return CurveSel{Q, nullptr}; }

// The plan of a batch is over whole blocks of CV_BLOCK targets, the target tile of every kernel of the three, and is sized by
// PlanSize with its rows read as targets: all blocks of the m (at least one), as many as keep the `capped` bytes of a block
// within `cap`; by rows the blocks that hold them, by bytes those that fit at `block` bytes each behind `fixed`.  blocks == 0:
// below one block.
constexpr int CV_BLOCK = 128;
struct TargetBlocks {
    i64 blocks, targets;                                            // per batch
};
static inline TargetBlocks target_block_plan(i64 m, PlanSize size, size_t block, size_t capped, size_t cap, size_t fixed = 0) {
    i64 most = (m + CV_BLOCK - 1) / CV_BLOCK;
    const i64 within = (i64)(cap / capped);
    most = most < within ? most : within;
    most = most < 1 ? 1 : most;
    i64 blocks = size.rows ? (size.rows + CV_BLOCK - 1) / CV_BLOCK : size.bytes < fixed ? 0 : (i64)((size.bytes - fixed) / block);
    blocks = blocks < most ? blocks : most;
    if (blocks < 1) return {0, 0};
    return {blocks, blocks * CV_BLOCK < m ? blocks * CV_BLOCK : m};
}
// run(q, count) for the batches [q, q + count) of the targets [0, m), `targets` a batch; the first failure ends the walk
template <typename Run>
static inline int for_target_batches(i64 m, i64 targets, Run run) {
    for (i64 q = 0; q < m; q += targets) {
        const int rc = run(q, m - q < targets ? m - q : targets);
        if (rc) return rc;
    }
    return SD_OK;
}
// run(q, tb) for the launches over the targets [q_begin, q_end): tb whole blocks from target q on, as many as keep a grid of
// `groups` workgroups a block within CV_LAUNCH_GROUPS, at least one
constexpr i64 CV_LAUNCH_GROUPS = (i64)1 << 30;
template <typename Run>
static inline int for_block_launches(i64 q_begin, i64 q_end, i64 groups, Run run) {
    i64 per = CV_LAUNCH_GROUPS / groups;                            // target blocks of a launch
    per = per < 1 ? 1 : per;
    for (i64 q = q_begin; q < q_end; q += per * CV_BLOCK) {
        const i64 left = (q_end - q + CV_BLOCK - 1) / CV_BLOCK;
        const int rc = run(q, left < per ? left : per);
        if (rc) return rc;
    }
    return SD_OK;
}

// ---- K20 squared L2 distances of curves, their k-th smallest and the h-modal sums (curve_dist.hip).  Only the h-modal sums
// have a plan over blocks: the tiles' partial sums of a batch. ----
constexpr int CD_WHAT_SQDIST = 0, CD_WHAT_HMODAL = 1, CD_WHAT_SELECT = 2;   // what a call forms: the `what` of the size functions
struct CurveDistPlan {
    int what;
    i64 targets;                                                    // per batch; 0: below the floor
    bool slab;                                                      // the selection keeps the n x n matrix
    size_t bytes;                                                   // SQDIST: none; HMODAL: the partial sums of a batch;
};                                                                  // SELECT: histogram and state, then the slab
CurveDistPlan curve_dist_plan(int what, i64 n, i64 m, PlanSize size);
int launch_curve_sqdist(const double *Y, i64 T, i64 n, CurveSel sel, i64 m, double *out, hipStream_t s);
int launch_hmodal_sums(const double *Y, i64 T, i64 n, CurveSel sel, i64 m, double g, double *out, void *ws, size_t ws_bytes,
                       hipStream_t s);
int launch_curve_sqdist_select(const double *Y, i64 T, i64 n, u64 k, double *out, void *ws, size_t ws_bytes, hipStream_t s);
// K21's pass 1 (the tile kernel's fourth epilogue): W[j * ldw + (q - q_begin)] = 1 / sqrt(D2[q][j]), 0.0 where D2 == 0.0, for the
// targets [q_begin, q_end) of the m; ldw a multiple of 128 that holds them, W 16-byte aligned
int launch_curve_weights(const double *Y, i64 T, i64 n, CurveSel sel, i64 m, i64 q_begin, i64 q_end, double *W, i64 ldw, hipStream_t s);

// ---- K21 functional spatial depth of curves (spatial_depth.hip): out[q] = S = |E[q]|^2, E[q][t] = sum_j w[q][j] (x[t] - Y[t][j]);
// field (null or m x T, target-major) = E.  The plan's blocks: the weights of a batch (n x targets, 8 n bytes a target) and its
// field (8 T bytes a target). ----
struct SpatialPlan {
    i64 targets;                                                    // per batch; 0: below the floor
    size_t weights, field;                                          // bytes of the two parts
    size_t bytes;                                                   // both
};
SpatialPlan spatial_plan(i64 T, i64 n, i64 m, PlanSize size);
// timepoints of the sum kernel's tile for a batch of `targets` targets on `cus` compute units: 64, or 32 where the 128 x 64
// tile would give fewer than two workgroups per unit
int spatial_time_tile(i64 T, i64 targets, i64 cus);
int launch_spatial_sums(const double *Y, i64 T, i64 n, CurveSel sel, i64 m, double *out, double *field, void *ws, size_t ws_bytes,
                        hipStream_t s);

// ---- K22 lens, spherical and beta-skeleton depth of curves (lens_depth.hip): out[q] = G = #{i < j : a + kappa b <= c and
// b + kappa a <= c}, a = D2(q, i), b = D2(q, j), c = D2(i, j) on K20's bits.  The plan: the n x n matrix in front, then the blocks:
// the rows of a batch of external targets (8 n bytes a target).  Sample targets read their rows from the matrix and go in one
// batch whatever the plan says. ----
constexpr i64 LN_MAX_N = 16384;                                     // the stored matrix is 2 GiB there; the caller checks
struct LensPlan {
    i64 targets;                                                    // external targets per batch; 0: below the floor
    size_t matrix, rows;                                            // bytes of the two parts
    size_t bytes;                                                   // both
};
LensPlan lens_plan(i64 n, i64 m, PlanSize size);
// the form (0 lens, 1 sphere, 2 general) of a kappa and an algo (0: by kappa, 1: general)
int lens_form(double kappa, int algo);
// tiles J of 64 sample curves that one workgroup of the count kernel walks, for a launch over `targets` targets
i64 lens_span(i64 n, i64 targets);
// K20's external distances of the targets [q_begin, q_end) of the m columns of Q: out[(q - q_begin) * n + j]
int launch_curve_sqdist_rows(const double *Y, i64 T, i64 n, const double *Q, i64 m, i64 q_begin, i64 q_end, double *out, hipStream_t s);
int launch_lens_counts(const double *Y, i64 T, i64 n, CurveSel sel, i64 m, double kappa, int algo, i64 *out, void *ws, size_t ws_bytes,
                       hipStream_t s);

// ---- K23 projections of curves on k directions (curve_project.hip): Z[r][i] = ((x_0 u_r0 + x_1 u_r1) + x_2 u_r2) + ..., X in
// either layout (st, sn), U k x T row-major, Z k x n.  The depths' records are K14's over the rows of Z, the outlyingness is
// K12's over them. ----
// Z[(r - r_first) * n + i] for the directions [r_first, r_end) and all n curves; no workspace
int launch_curve_project(const double *X, i64 T, i64 n, i64 st, i64 sn, const double *U, i64 r_first, i64 r_end, double *Z,
                         hipStream_t s);
// The plan of sd_rp_depth_sums: a chunk of `rows` rows of Z in front (z bytes), then K14's stage 1 for them.  Sized by
// PlanSize with its rows read as rows of Z; rows == 0: below the floor.
struct RpDepthPlan {
    i64 rows;                                                       // of Z per chunk
    size_t z;                                                       // bytes of the chunk, padded to 256
    size_t bytes;                                                   // the whole of it
};
RpDepthPlan rp_depth_plan(i64 n, i64 k, int route, PlanSize size);
int launch_rp_depth_sums(const double *X, i64 T, i64 n, i64 st, i64 sn, const double *U, i64 k, const i64 *targets, i64 m,
                         int route, i64 *out, void *ws, size_t ws_bytes, hipStream_t s);
size_t rp_outlyingness_workspace_bytes(i64 n, i64 k);
size_t rp_outlyingness_min_workspace_bytes(i64 n);
int launch_rp_outlyingness(const double *X, i64 T, i64 n, i64 st, i64 sn, const double *U, i64 k, const i64 *targets, i64 m,
                           double *out, void *ws, size_t ws_bytes, hipStream_t s);

}  // namespace sd
