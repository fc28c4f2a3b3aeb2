// point_select.h -- which rows of a point cloud a target is set against (internal; K4, K5, K7, K10 pairwise, K11, K12, K13).
//
// Every point-cloud depth is asked for in three forms, one launch each:
//   rows     -- row targets[q] of P (NULL: row q) inside P: the sample is all n rows, the target among them;
//   external -- the point Q[q] (m x d) inside P u {Q[q]}: the sample is all n rows, the target is none of them
//               (the homogeneity coefficients' depth of a point of G inside F u {g}, homogeneity.py:172-186);
//   blocks   -- the LAST member of block q (members int32[m][bs], padded with -1 AT THE END) inside that block: the
//               sample is the block's rows, others first (the K-block sampled estimator, _pointcloud.py:107-121).
//               A block's members are the entries before its first -1; a block without members has no target.
// K4, K5, K7 and K13 work on the target's OTHERS (the sample without the target's row); K10 and K11 count the whole sample,
// and an external target counts itself on top (self); K12 takes the median and the MAD of the whole sample, an external
// target's projection inserted.
#pragma once
#include "sd_common.h"

namespace sd {

struct PointSel {
    const i64 *targets;
    const double *Q;
    const int *members;
    int bs;
};

static inline PointSel select_rows(const i64 *targets) { return PointSel{targets, nullptr, nullptr, 0}; }
static inline PointSel select_external(const double *Q) { return PointSel{nullptr, Q, nullptr, 0}; }
static inline PointSel select_blocks(const int *members, int bs) { return PointSel{nullptr, nullptr, members, bs}; }

// the largest sample of a call (rows of P, the target's own included where it is one) and the most others a target has
static inline i64 sel_cnt_max(const PointSel &sel, i64 n) { return sel.members ? (i64)sel.bs : n; }
static inline i64 sel_others_max(const PointSel &sel, i64 n) { return sel.members ? (i64)sel.bs - 1 : sel.Q ? n : n - 1; }

#ifdef __HIPCC__
// One target of a call.  The sample is rows mem[0 .. cnt - 1] of P, or rows 0 .. cnt - 1 when mem is null.
struct PointView {
    const double *x;                                                // the target's coordinates (d of them)
    const int *mem;                                                 // the block's members, or null
    i64 tg;                                                         // the target's row in P; -1: external, or an empty block
    i64 cnt;                                                        // sample rows in P

    __device__ __forceinline__ i64 others() const { return tg >= 0 ? cnt - 1 : cnt; }
    // row of the i-th other, i < others(): the sample in order, the target skipped (a block's target is its last member)
    __device__ __forceinline__ i64 other(i64 i) const {
        if (mem) return mem[i];
        if (tg < 0) return i;
        return i < tg ? i : i + 1;
    }
    __device__ __forceinline__ int self() const { return !mem && tg < 0 ? 1 : 0; }   // the target counts itself on top
};

// members of a block: the entries before the first -1
__device__ __forceinline__ int block_count(const int *mem, int bs) {
    int c = 0;
    while (c < bs && mem[c] >= 0) ++c;
    return c;
}

// the same number found by the NT threads of a workgroup together (two barriers; every thread gets it)
template <int NT>
__device__ __forceinline__ int block_count_coop(const int *mem, int bs, int *s_cnt) {
    if (threadIdx.x == 0) *s_cnt = bs;
    __syncthreads();
    int first = bs;
    for (int i = threadIdx.x; i < bs && first == bs; i += NT)
        if (mem[i] < 0) first = i;
    if (first < bs) atomicMin(s_cnt, first);
    __syncthreads();
    return *s_cnt;
}

// target q of the call; c = the number of members of block q (blocks form only).  P is n x d.  An empty block gets
// cnt = 0, tg = -1 and a readable x (row 0) that no result depends on.
__device__ __forceinline__ PointView point_view_counted(const PointSel &sel, const double *P, i64 n, int d, i64 q, int c) {
    PointView v;
    if (sel.members) {
        v.mem = sel.members + q * sel.bs;
        v.cnt = c;
        v.tg = c > 0 ? (i64)v.mem[c - 1] : -1;
        v.x = P + (c > 0 ? v.tg : 0) * d;
    } else if (sel.Q) {
        v.mem = nullptr;
        v.cnt = n;
        v.tg = -1;
        v.x = sel.Q + q * d;
    } else {
        v.mem = nullptr;
        v.cnt = n;
        v.tg = sel.targets ? sel.targets[q] : q;
        v.x = P + v.tg * d;
    }
    return v;
}

// resolved by one thread for itself
__device__ __forceinline__ PointView point_view(const PointSel &sel, const double *P, i64 n, int d, i64 q) {
    return point_view_counted(sel, P, n, d, q, sel.members ? block_count(sel.members + q * sel.bs, sel.bs) : 0);
}

// resolved by a workgroup of NT threads (sel is a kernel argument, so the branch around the barriers is uniform)
template <int NT>
__device__ __forceinline__ PointView point_view_coop(const PointSel &sel, const double *P, i64 n, int d, i64 q, int *s_cnt) {
    return point_view_counted(sel, P, n, d, q,
                              sel.members ? block_count_coop<NT>(sel.members + q * sel.bs, sel.bs, s_cnt) : 0);
}
#endif

}  // namespace sd
