/*
 * statdepth_hip_projections.h -- K23: projections of curves on a fixed set of directions and the random projection
 * depths, a companion of statdepth_hip.h.
 *
 * Why a second header.  tests/workspace_contract.py and the tests built on it tie every stream-taking symbol of
 * statdepth_hip.h (and of statdepth_amd/_native.py's SIGNATURES) to a row of their tables and to a case of
 * tests/test_workspace_contract_gpu.py.  The change that added K23 was not to touch those files, so its entry points are
 * declared here, bound from _native.PROJECTION_SIGNATURES next to the first table, and run through the same contract
 * proxy in their own test file (tests/test_rp_depths_gpu.py).  A later change that may touch the contract tables folds
 * this header into statdepth_hip.h and the second table into the first.
 *
 * Everything statdepth_hip.h says holds here unchanged: the conventions (device pointers, x(t,i) = X[t*st + i*sn] in either
 * layout, `targets` or NULL with m == n, SD_OK or an error code with sd_last_error()), the ABI version (still 1), and the
 * "Caller memory" contract: `ws` may hold any bytes on entry, nothing in it is needed after the call, it is passed 256-byte
 * aligned, no byte is written outside [ws, ws + ws_bytes) or outside the documented extent of an output, outputs may hold
 * any bytes on entry, calls enqueue and return.
 *
 * Definition.  X is T x n fp64 in either layout, U is k x T fp64 row-major (a direction per row).  For curve i and
 * direction r
 *   z_r(i) = ((x_0 u_r0 + x_1 u_r1) + x_2 u_r2) + ...      timepoints in increasing order,
 * every product and every sum rounded separately to fp64 (no FMA, no contraction), the first term the product alone (not
 * 0 + product, so a sum of -0.0 terms is -0.0).  The numpy loop z = X[0]*u[0]; for t in 1 .. T-1: z = z + X[t]*u[t] gives
 * the same bits, and for T <= 8 they are the bits of K10's and K12's projection of a point of R^T.  Unlike the other curve
 * kernels this one reads both layouts in place: no time-major copy is made.  Finite data with |x|, |u| <= 2^500 and
 * T < 2^23 cannot overflow (the host layer refuses anything else; the library takes its arrays as they are).
 * Z = (z_r(i)) is k x n, direction-major: Z[r*n + i].
 *
 * Records.  With K14's A_r, B_r (the strict counts over the other n - 1 curves, ties in neither) taken on row r of Z
 * instead of a timepoint, out[q] is K14's record of five int64 over the k rows of Z,
 *   SA = sum_r A,   SB = sum_r B,   SF = sum_r |2 A - n|,   SM = sum_r max(A, B),   MM = max_r max(A, B),
 * and the depths are formed on the host in fp64, one expression each, the division last:
 *   'rp_halfspace'   (n k - SM) / (n k)    mean over the directions of the univariate Tukey depth (random projection depth);
 *   'rp_fm'          1 - SF / (2 n k)      mean over the directions of 1 - |1/2 - F_r|, F_r the "<=" empirical CDF; formed as
 *                                          K14 forms Fraiman-Muniz: (2 n k - SF) / (2 n k), integers up to the division;
 *   'random_tukey'   (n - MM) / n          minimum over the directions: the random Tukey depth.
 * Outlyingness.  O(q) = max over r of |z_r(q) - med_r| / mad_r with K12's median, MAD (no factor), division and zero
 * cases on row r of Z (statdepth_hip.h, K12: a numerator of 0 gives 0 whatever the MAD, a positive numerator over a MAD of
 * 0 gives +inf); 'rp_projection' is 1 / (1 + O) on the host.
 * A cloud of n points with any number T of features is a set of n curves at T timepoints: 'random_tukey' and
 * 'rp_projection' over a direction array U are then the halfspace and the projection depth of K10 and K12 (n - MM is
 * sd_halfspace_counts' integer), without their limit of 8 features.
 *
 * Refusals of the three compute entry points, all before any device work: SD_ERR_INVALID for NULL X, U or out, T < 1,
 * k < 1, n < 2 (sd_curve_projections: n < 1), an unknown algo, strides that are neither layout, m < 0 or targets == NULL
 * with m != n; SD_ERR_UNSUPPORTED for 2^31 or more curves, timepoints or directions, for algo = 1 with more than 16 384
 * curves, or for more than 10^14 multiply-adds plus comparisons (T n k + k n (1 + log2 n)); SD_ERR_WORKSPACE below the
 * floor.
 */
#ifndef STATDEPTH_HIP_PROJECTIONS_H
#define STATDEPTH_HIP_PROJECTIONS_H

#include "statdepth_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out: k x n fp64 (device), out[r*n + i] = z_r(i).  One tiled kernel (csrc/curve_project.hip): a workgroup of 256 threads
 * owns 128 curves x 64 directions, panels of 16 timepoints of X and U in LDS, an 8 x 4 accumulator tile per thread that is
 * never split over t; no atomics, so the bits do not depend on the tiling, the layout or the launch shape.  Needs no
 * workspace: sd_curve_projections_workspace_bytes returns 0 and ws may be NULL. */
size_t sd_curve_projections_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t k);
int sd_curve_projections(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *U, int64_t k,
                         double *out, void *ws, size_t ws_bytes, void *stream);

/* out: m x 5 int64 (device), the records.  A chunk of rows of Z is projected into the workspace and handed to K14's stage 1
 * and fold as rows of curves are (algo 0 auto, 1 image: n <= 16 384, 2 sort); the chunks follow each other on the stream.
 * The workspace holds the chunk (8 n bytes a row) and K14's own need for it: sd_rp_depth_workspace_bytes recommends a size
 * (all k rows whenever Z is within 1 GiB), sd_rp_depth_min_workspace_bytes is the floor (one row).  The integers do not
 * depend on ws_bytes.  Both return 0 for a shape or algo the call refuses. */
size_t sd_rp_depth_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t k, int64_t m, int algo);
size_t sd_rp_depth_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t k, int64_t m, int algo);
int sd_rp_depth_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *U, int64_t k,
                     const int64_t *targets, int64_t m, int algo, int64_t *out, void *ws, size_t ws_bytes, void *stream);

/* out: m fp64 (device), O(q).  Per chunk of directions: the rows of Z, K10's row sort of a copy of them, K12's selection of
 * med_r and mad_r from the sorted rows, then a thread per target takes the maximum of o_r over the chunk from the unsorted
 * Z; the first chunk starts out[], later ones fold into it on the stream.  About 32 n bytes a direction of a chunk:
 * sd_rp_outlyingness_workspace_bytes recommends a size (2^23 values a chunk), sd_rp_outlyingness_min_workspace_bytes is
 * the floor (one direction).  The maximum is exact and order-free: the result does not depend on ws_bytes. */
size_t sd_rp_outlyingness_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t k, int64_t m);
size_t sd_rp_outlyingness_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t k, int64_t m);
int sd_rp_outlyingness(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *U, int64_t k,
                       const int64_t *targets, int64_t m, double *out, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* STATDEPTH_HIP_PROJECTIONS_H */
