// rank_fold.h -- the skeleton of the kernels that fold an image of per-(row, curve) rank words over the rows into totals per
// target (mbd_rank_fold.hip, rank_depths.hip, the finalize kernels of mbd_rank_bucket.hip, rank_reduce_kernel of mbd_rank.hip):
//   * a block is X targets (or X groups of W neighbouring targets) x SLICES row slices, thread = y * X + x;
//   * fold_rows: slice y streams the rows y, y + SLICES, ... with U independent loads in flight, then a ragged tail;
//   * fold_store / fold_store_w: an LDS tree over the slices, out = on the first batch of a call and out += on later ones
//     (a target has one owner and the batches follow each other on the stream: no atomics);
//   * fold_pair16 / fold_ab2: what a word of the two pair images adds to a target's band counts.
// What a load is and what a use does are the caller's; so are the LDS array and its padding.  Everything here is inlined.
#pragma once
#include "sd_common.h"
#include "rank_routes.h"
#include "rank_big_common.h"

namespace sd {

// a load of the row loop that needs the row's NaN count next to its word(s)
template <typename W>
struct FoldLoad {
    W w;
    u32 nn;
};

// rows y, y + SLICES, ... < rows: U loads issued together, then their U uses; then single rows.
// load(row) -> V, use(const V &, row).
template <int SLICES, int U, typename Load, typename Use>
__device__ __forceinline__ void fold_rows(i64 rows, int y, Load load, Use use) {
    i64 r = y;
    for (; r + SLICES * (U - 1) < rows; r += SLICES * U) {
        decltype(load(r)) v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = load(r + SLICES * u);
#pragma unroll
        for (int u = 0; u < U; ++u) use(v[u], r + SLICES * u);
    }
    for (; r < rows; r += SLICES) use(load(r), r);
}

// One value per thread: *o (=|+=, first) the sum over the slices of thread column x; slice 0 stores where `live`.
// Whole blocks call this (two barriers).
template <int SLICES, int PITCH>
__device__ __forceinline__ void fold_store(u64 (&red)[SLICES][PITCH], int x, int y, u64 v, bool live, u64 *o, int first) {
    red[y][x] = v;
    __syncthreads();
    if (y == 0 && live) {
        u64 tot = 0;
#pragma unroll
        for (int k = 0; k < SLICES; ++k) tot += red[k][x];
        if (first) *o = tot;
        else *o += tot;
    }
    __syncthreads();
}

// W neighbouring targets per thread: red holds SLICES rows of ROWPITCH words, thread column x its W values at x * XPITCH.
// The first X * W threads store: thread t owns target q0 + t of the block (q0: the block's first), out[(q0 + t) * stride].
template <int SLICES, int X, int W, int XPITCH, int ROWPITCH>
__device__ __forceinline__ void fold_store_w(u64 *red, int x, int y, const u64 (&v)[W], i64 q0, i64 m, u64 *out, int stride,
                                             int first) {
    static_assert(XPITCH >= W && ROWPITCH >= X * XPITCH, "the threads' values do not overlap");
#pragma unroll
    for (int c = 0; c < W; ++c) red[y * ROWPITCH + x * XPITCH + c] = v[c];
    __syncthreads();
    const int t = threadIdx.x;
    if (t < X * W) {
        const int at = (t / W) * XPITCH + (t % W);
        const i64 q = q0 + t;
        if (q < m) {
            u64 tot = 0;
#pragma unroll
            for (int k = 0; k < SLICES; ++k) tot += red[k * ROWPITCH + at];
            if (first) out[q * stride] = tot;
            else out[q * stride] += tot;
        }
    }
    __syncthreads();
}

// ---- the 16-bit pair image: B | A << 16, AB_SPECIAL where the curve is NaN ----
template <int J>
__device__ __forceinline__ void fold_pair16(u32 ab, u32 nn, i64 n, u64 (&acc)[JMAX - 1]) {
    if (ab != AB_SPECIAL) band_counts_add<J>(ab >> 16, ab & 0xFFFFu, nn, (u64)(n - 1), acc);
}

// ---- the AB2 image (rank_big_common.h) ----
// does the B word w send its reader to the A image?
__device__ __forceinline__ bool ab2_tied(u32 w) { return w != AB2_NAN && (w & AB2_TIE) != 0; }
// the word of (row, curve) idx: from the half-word image where there is one (min(A, B) of an untied key stands for B: the
// counts are symmetric in A and B), else / on its marker from the B image
__device__ __forceinline__ u32 ab2_word(const AB2 &ab, i64 idx) {
    if (ab.H) {
        const u32 h = ab.H[idx];
        if (h != (u32)AB2_H_WORD) return h;
    }
    return ab.B[idx];
}
// the same for a half word h already loaded
__device__ __forceinline__ u32 ab2_word(u32 h, const u32 *__restrict__ B, i64 idx) { return h == (u32)AB2_H_WORD ? B[idx] : h; }
// a_word: where the key's A stands, read for a tied key only
template <int J>
__device__ __forceinline__ void fold_ab2(u32 w, u32 nn, i64 n, const u32 *a_word, u64 (&acc)[JMAX - 1]) {
    if (w == AB2_NAN) return;
    const u32 B = w & ~AB2_TIE;
    if (J == 2 && nn == 0 && !(w & AB2_TIE)) {
        // untied key of a NaN-free row: A + B = n - 1, and C(A + B, 2) - C(A, 2) - C(B, 2) = A * B
        acc[0] += (u64)B * (u64)((u32)n - 1u - B);
        return;
    }
    const u32 A = (w & AB2_TIE) ? *a_word : (u32)n - nn - 1u - B;            // tied keys carry their A
    band_counts_add<J>(A, B, nn, (u64)(n - 1), acc);
}

}  // namespace sd
