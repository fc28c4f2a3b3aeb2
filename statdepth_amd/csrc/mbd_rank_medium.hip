// mbd_rank_medium.hip -- M: pair image of rows of 16 384 < n <= 40 960 curves (the "medium" sizes a 2- to 4-GPU time-sharded
// step sees: n = N * 10^4) as 2 or 3 column blocks through ONE workgroup.
//
// Ranks are additive over column blocks: per row each block in turn is histogrammed, prefix-summed and scattered (RbRow,
// rank_bucket_row.h: the build of rank_external_kernel), and EVERY key of the row -- the block's own (still in registers) and
// the other blocks' (read again: the row sits in L2) -- looks up its bucket there: B += base + #(y < x), A += n_valid - base -
// #(y <= x) (a key meets itself in its own block: `<=` keeps it out of A, `<` out of B).  The running counts wait in the
// image itself (this thread's own words).  One build and NBLK look-ups per key: about the bucket kernel's cost per key at two
// blocks, against three passes over global memory on the large-n route.  Output as the bucket kernel's image mode
// (B | A << 16, 0xFFFFFFFF for NaN; counts < 2^16), folded by the same rank_accumulate kernels.
#include "sd_common.h"
#include "rank_routes.h"
#include "rank_bucket_row.h"

namespace sd {

constexpr int RB_MEDIUM_MAXN = 40960;          // 2 or 3 blocks (measured: 4 blocks lose to the large-n route)

template <int NT, int E, int LNB>
__global__ __launch_bounds__(NT) void rank_medium_image_kernel(const double *__restrict__ Y, i64 n64, i64 row0, i64 rows, int nblk,
                                                               u32 *__restrict__ AB, u32 *__restrict__ nnan_img) {
    // a bucket of 16 keys or more is tie-heavy data more often than a dense cluster (see rank_bucket_kernel)
    using Row = RbRow<NT, E, LNB, 4, true>;
    constexpr int NB = Row::NB;
    extern __shared__ double Sm[];
    const int n = (int)n64;
    constexpr int BS = E * NT;                                        // block j: curves [j BS, min((j + 1) BS, n))
    const int t0 = threadIdx.x;
    const double INF = __builtin_huge_val();
    const double QNAN = __builtin_nan("");
    const int DUMMY = Row::C::dummy_pos(BS);
    int t = t0;
    Row blk(Sm);
    for (i64 r = blockIdx.x; r < rows; r += gridDim.x) {
        t = t0;
        asm volatile("" : "+v"(t));                                   // per-row opaque thread id (see rank_bucket_kernel)
        blk.thread(t);
        const double *row = Y + (row0 + r) * n;
        u32 *img = AB + r * n;                                        // B | A << 16 so far, per key
        u32 nn_tot = 0;
        for (int jb = 0; jb < nblk; ++jb) {
            const int boff = jb * BS;
            const int bsz = n - boff < BS ? n - boff : BS;
            double kk[E];
#pragma unroll
            for (int e = 0; e < E; ++e) kk[e] = (t + e * NT < bsz) ? row[boff + t + e * NT] : QNAN;
            const typename Row::Built built = blk.build(kk, bsz, DUMMY);   // (0) - (3), barriers 1 - 4
            const u32 nv = built.nv;
            const bool flat = built.flat;                             // every finite key of the block holds one value
            nn_tot += (u32)bsz - nv;                                  // pad slots beyond the block are NaN too: not in bsz
            // Tie-heavy rows (values on a grid, duplicated curves): if every bucket of the block holds ONE value -- every key
            // equals its bucket's first -- a look-up is a compare with that value, not a walk over hundreds of members
            bool allpure = false;                                     // block-uniform
            if (built.trypure && !flat) {
                __syncthreads();
                bool pure = true;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const u32 b = built.bs[e] & 0xFFFFu;
                    if (b < (u32)NB) pure = pure && (blk.S[blk.H16[b]] == kk[e]);
                }
                allpure = __syncthreads_and(pure) != 0;
            }
            u32 flat_lo = 0, flat_hi = 0;                             // a flat block's -inf / +inf keys
            if (flat) {
                u32 ml = 0, mh = 0;
#pragma unroll
                for (int e = 0; e < E; ++e) { ml += kk[e] == -INF; mh += kk[e] == INF; }
                for (int k2 = 0; k2 < E; ++k2) {                      // block-wide sums, one count at a time (rare path)
                    flat_lo += __syncthreads_count(k2 < (int)ml);
                    flat_hi += __syncthreads_count(k2 < (int)mh);
                }
            }
            __syncthreads();                                          // barrier 5
            // ---- (4) every key of the row against the members of its bucket in this block ----
            // (a six-key window read ahead of the compares, as in rank_bucket_kernel, was measured here and changed nothing
            // at E = 10 and cost 15 % at E = 15: the look-ups are not what this kernel waits for -- its global loads are)
            auto lookup = [&](double x) -> u32 {
                if (flat) {                                           // block-uniform: one bucket of equal keys (and infinities)
                    const u32 neq = nv - flat_lo - flat_hi;
                    const u32 less = (x > -INF ? flat_lo : 0u) + (x > built.lo ? neq : 0u);
                    const u32 le = flat_lo + (x >= built.lo ? neq : 0u) + (x >= INF ? flat_hi : 0u);
                    return (x == x) ? (less | ((nv - le) << 16)) : 0u;
                }
                u32 c = 0;
                if (x == x) {
                    const u32 b = built.bucket_of(x);
                    const u32 base = blk.H16[b], end = blk.H16[b + 1];
                    u32 less = 0, le = 0;
                    if (allpure) {                                    // block-uniform: one value per bucket
                        const double y = blk.S[base < end ? base : 0u];
                        less = (base < end && y < x) ? end - base : 0u;
                        le = (base < end && y <= x) ? end - base : 0u;
                    } else
#pragma unroll 1
                    for (u32 j = base; j < end; ++j) {
                        const double y = blk.S[j];
                        less += (y < x) ? 1u : 0u;
                        le += (y <= x) ? 1u : 0u;
                    }
                    c = (base + less) | ((nv - base - le) << 16);
                }
                return c;
            };
            const bool first = jb == 0, last = jb == nblk - 1;
            for (int ib = 0; ib < nblk; ++ib) {                       // block-uniform
                const int ioff = ib * BS;
                const int isz = n - ioff < BS ? n - ioff : BS;
                // the other block's keys and the running counts first, all in flight together (one at a time they cost a
                // trip to L2 per key: 48 us per row of 20 000 instead of 30), then the look-ups, then the stores
                double xk[E];
                u32 cw[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const bool in = t + e * NT < isz;
                    xk[e] = ib == jb ? kk[e] : (in ? row[ioff + t + e * NT] : QNAN);
                    cw[e] = (!first && in) ? img[ioff + t + e * NT] : 0u;
                }
#pragma unroll
                for (int e = 0; e < E; ++e) cw[e] += lookup(xk[e]);
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (t + e * NT < isz) img[ioff + t + e * NT] = (last && !(xk[e] == xk[e])) ? AB_SPECIAL : cw[e];
            }
            __syncthreads();                                          // barrier 6: S and the bases have been read
            blk.clear();
        }
        if (t == 0) nnan_img[r] = nn_tot;
    }
}

// medium sizes: pair image through 2 or 3 column blocks of at most 16 384 curves per workgroup (10^7 keys, host call
// included: n = 20 000: 0.159 ms against 0.223 on the large-n route; 30 000: 0.208 / 0.228; 40 000: 0.228 / 0.239;
// 60 000 as four blocks: 0.355 / 0.243 -- not taken)
bool rank_medium_supported(i64 n) { return n > 16384 && n <= RB_MEDIUM_MAXN; }
int launch_rank_medium_image(const double *Y, i64 n, i64 row0, i64 rows, u32 *AB, u32 *nnan, hipStream_t s) {
    if (!rank_medium_supported(n)) return fail(SD_ERR_UNSUPPORTED, "medium image kernel covers 16384 < n <= %d", RB_MEDIUM_MAXN);
    const int cus = device_cus();
    const int G = (int)(rows < cus ? rows : cus);
    const int nblk = (int)((n + 16383) / 16384);                                     // fewest blocks ...
    const int E = (int)((n + (i64)nblk * 1024 - 1) / ((i64)nblk * 1024));             // ... of equal size, whole thousands
#define RB_MD(E_)                                                                                                        \
    case E_:                                                                                                             \
        return rb_launch(rank_medium_image_kernel<1024, E_, rb_lnb(E_, 3)>, G, 1024,                                     \
                         RBCfg<1024, E_, rb_lnb(E_, 3), 3>::lds_bytes(E_ * 1024), s, Y, n, row0, rows, nblk, AB, nnan);
    switch (E) {
        RB_MD(9) RB_MD(10) RB_MD(11) RB_MD(12) RB_MD(13) RB_MD(14) RB_MD(15) RB_MD(16)
    }
#undef RB_MD
    return fail(SD_ERR_UNSUPPORTED, "medium image kernel: no instantiation for n=%lld", (long long)n);
}

}  // namespace sd
