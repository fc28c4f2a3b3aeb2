// halfspace_sort.h -- K10's bit-specified projection and its sorted rows, shared with K12 (internal).
//
// launch_hs_sort_chunk (halfspace.hip) projects the sample on a chunk of directions and sorts every direction's
// projections: hs_project_kernel, hs_tile_sort_kernel, then hs_partition_kernel / hs_merge_kernel passes between two
// buffers.  K10 ranks the sorted rows (halfspace.hip), K12 selects medians from them (projection.hip), K14 sorts rows
// of curves with launch_hs_sort_rows and ranks them into a pair image (rank_depths.hip).
#pragma once
#include "sd_common.h"

namespace sd {

constexpr int HS_THREADS = 256;
constexpr int HS_TILE = 2048;                                      // values per sort / merge tile
constexpr i64 HS_CHUNK_VALUES = (i64)1 << 25;                      // projected values per chunk (one row when n is larger)
constexpr i64 HS_REC_VALUES = (i64)1 << 23;                        // ... of the recommended workspace

static inline int hs_ntiles(i64 n) { return (int)((n + HS_TILE - 1) / HS_TILE); }

// the buffers of a chunk of kc directions: keys and indices twice (a merge pass reads one pair and writes the other),
// and one merge-path split per (direction, tile)
struct HsSortBuffers {
    double *K[2];
    u32 *I[2];
    int *part;
};
constexpr int HS_SORT_CARVES = 5;                                  // take() calls of hs_sort_carve
static inline size_t hs_sort_bytes_per_direction(i64 n) { return (size_t)n * 24 + (size_t)hs_ntiles(n) * 4; }
static inline bool hs_sort_carve(Carver &cv, i64 n, i64 kc, HsSortBuffers &b) {
    b.K[0] = (double *)cv.take((size_t)kc * n * 8);
    b.K[1] = (double *)cv.take((size_t)kc * n * 8);
    b.I[0] = (u32 *)cv.take((size_t)kc * n * 4);
    b.I[1] = (u32 *)cv.take((size_t)kc * n * 4);
    b.part = (int *)cv.take((size_t)kc * hs_ntiles(n) * 4);
    return b.K[0] && b.K[1] && b.I[0] && b.I[1] && b.part;
}
// directions per chunk that `bytes` hold, at most k and at most HS_CHUNK_VALUES / n (one at least)
static inline i64 hs_chunk_directions(size_t bytes, size_t per_direction, i64 n, i64 k) {
    i64 kc = (i64)(bytes / per_direction);
    const i64 cap = HS_CHUNK_VALUES / n < 1 ? 1 : HS_CHUNK_VALUES / n;
    kc = kc > cap ? cap : kc;
    return kc > k ? k : kc;
}

// Rows 0 .. kk - 1 of Z[r][i] = z_r(p_i), r counted from the first direction of U (kk x d), each sorted ascending in
// b.K[*src] (kk x n), the values' sample rows beside them in b.I[*src].  d in [1, 8].
int launch_hs_sort_chunk(const double *P, i64 n, int d, const double *U, int kk, const HsSortBuffers &b, int *src,
                         hipStream_t s);
// The same sort of kk rows of n values that the caller has put into b.K[0] (the second half of launch_hs_sort_chunk).
int launch_hs_sort_rows(i64 n, int kk, const HsSortBuffers &b, int *src, hipStream_t s);

#ifdef __HIPCC__
template <int D>
__device__ __forceinline__ double hs_proj(const double (&x)[D], const double (&u)[D]) {
    double z = __dmul_rn(x[0], u[0]);
#pragma unroll
    for (int e = 1; e < D; ++e) z = __dadd_rn(z, __dmul_rn(x[e], u[e]));
    return z;
}
#endif

}  // namespace sd
