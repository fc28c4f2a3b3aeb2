// tvd.hip -- K17: total variation depth and modified shape similarity of curves (Huang & Sun 2019).
//
// Definition.  n curves at T timepoints, time-major Y[t][i], no NaN.  For a target q the whole sample counts, q included:
//   a_t = #{j : Y[t][j] <= Y[t][q]}                                  (= n - A of K14, 1 <= a_t <= n)
//   c_t = #{j : Y[s][j] <= Y[s][q] and Y[t][j] <= Y[t][q]},  s = t - 1, for t >= 1.
// Total variation depth: TVD(q) = (1/T) sum_t a_t (n - a_t) / n^2.  The device returns the integer SD = sum_t a_t (n - a_t)
// (<= T n^2 / 4, fits int64); the host divides once.
// Shape similarity at step t >= 1: S_t = (n c_t - a_s a_t)^2 / (a_s (n - a_s) a_t (n - a_t)), the squared phi coefficient of
// the 2 x 2 table of the indicators at s and t (= Var(E[R_t | R_s]) / Var(R_t) of the paper).  Where the denominator is 0
// (a_s = n or a_t = n) the numerator is 0 as well and S_t = 1: our convention.  In fp64: e = (double)(n c_t - a_s a_t), exact
// (|e| <= n^2 < 2^53); S_t = (e * e) / ((double)(a_s (n - a_s)) * (double)(a_t (n - a_t))), the integer products in int64:
// three rounded operations.
// Modified shape similarity: MSS(q) = sum_{t>=1} v_t S_t, v_t = |Y[t][q] - Y[t-1][q]| / sum_u |Y[u][q] - Y[u-1][q]|.  The
// device returns SS = sum S_t, SN = sum |D_t| S_t, SW = sum |D_t| per target; the host forms SN / SW, or SS / (T - 1) for a
// constant curve (SW = 0).
//
// LDS route (n <= 16 384; what auto runs there).  Stage 1 is K14's pair image (launch_rank_pair_images, route 1): u32 words
// B | A << 16 per (row, curve), B the number strictly below.  Y[s][j] <= Y[s][i] iff B_j(s) <= B_i(s), so
//   c_i = #{j : B_j(s) <= B_i(s) and B_j(t) <= B_i(t)}:  a weak 2-D dominance count of n integer points.
// tvd_dominance_kernel, one workgroup per row pair, what we chose: a sqrt(n) x sqrt(n) block histogram with a 2-D prefix
// sum, plus two partial scans per point.
//   1  Counting scatter, once per row: curve i takes the position xp = B_i + (an LDS atomic counter of the value B_i), so
//      the curves tied at a row fill the positions [B, a) in some order and xp is a permutation of 0 .. n - 1; yp likewise at
//      row t.  With mx = a_s(i) - 1 and my = a_t(i) - 1, the last position of i's own run of ties,
//          c_i = #{j : xp_j <= mx_i and yp_j <= my_i}
//      whatever order the ties took: the count covers the whole prefix up to a_s(i), not up to the point's own position, and
//      exact duplicates at both rows count each other.
//   2  Strips of 128 positions in x and in y: TX(bx, k) = yp of the curve at xp = 128 bx + k, TY(by, k) = xp of the curve
//      at yp = 128 by + k, H[bx][by] = curves per cell (two u16 cells per u32 atomic; a cell holds at most 128), then the
//      inclusive 2-D prefix sum of H in place, by wave scans along the rows and along the columns.
//   3  Per curve, with qbx = mx >> 7 and qby = my >> 7:  the cells left of and below both strips from H, plus the 128
//      entries of x-strip qbx with k <= mx & 127 and yp <= my, plus the 128 entries of y-strip qby with k <= my & 127
//      and xp < 128 qbx.  The three parts are disjoint and cover the quadrant.
//   The curves a wave holds sit in arbitrary strips, and a strip-major layout would put their reads of entry k on one bank.
//   The strips are stored in groups of four entries instead (tvd_entry: u64 word (k >> 2) * SP + strip), so one 8-byte
//   read brings four entries and the reads of a wave fall on consecutive words; curves of one strip broadcast.  The four
//   are compared in their 16-bit fields at once: entries are at most 0x7FFF (a missing entry of the last strip is 0x7FFF),
//   so the field 0x8000 + h - v borrows from no neighbour and has bit 15 set iff v <= h, and a population count adds the
//   flags -- whole groups below the group that holds the curve's position limit, no group above it, and that one group with
//   the flags past the limit shifted out.  64 reads per curve and row pair.
//   LDS: (256 SP + nb SP) u16 with nb = ceil(n / 128), SP = nb | 1: 99 072 bytes at n = 16 384 (one workgroup per CU),
//   52 932 at 10 000 (three of 640 threads); the scatter's n u32 counters lie under TX and TY, which are written after
//   it.  The kernel is bound by vector instruction issue (SQ counters, DESIGN section 3 K17: several hundred instructions per
//   curve and row pair; the LDS is busy a third of the time, half of that in bank conflicts of the random strips), not by
//   memory: 3 n words in, n / 2 out per row pair.  No scratch, no inline assembly.  Measured (profiles/tvd_times.txt):
//   10 000 x 1 000, every curve a target, 0.35 ms for the call, of which this kernel 0.25 ms.
//   Stored: C[row][i] = c - 1 as u16 (c >= 1: the curve counts itself; c - 1 <= 16 383), plain stores.
// TvdImageFold is the RankImageConsumer of the route: per batch of rows [row0, row0 + rows) it runs the dominance kernel
// on the pairs (t - 1, t) of the batch -- the pair that straddles the boundary reads its first row from `carry`, the last
// image row of the batch before, n words kept in the workspace -- then tvd_fold_kernel, then copies the batch's last row
// into `carry`.  Every pair runs exactly once for any batch size, one row per batch included.
//
// tvd_fold_kernel (modelled on rank_depth_fold_kernel): block = 64 targets x 16 row slices; slice y owns the rows with
// t % 16 == y of EVERY batch and keeps its record (SD, SS, SN, SW) in the workspace between batches, so a (target, slice)
// pair has one owner, the batches follow each other on the stream, there are no atomics, and each slice adds its rows in
// ascending order whatever the batch size: the doubles, like the integers, do not depend on the workspace size.
// tvd_finish_kernel adds the 16 slices of a target in slice order.
//
// Pairwise route (any n < 2^31; the cross-check of the LDS route and the route above 16 384 curves): tvd_pairwise_kernel
// reads only the doubles.  256 targets a block against LDS tiles of 1024 curves of the rows s and t; a_s, a_t and c_t are
// counted by comparison and fed to the same arithmetic, the same 16 slices and the same finish.  O(T n m).  A merge route
// in global memory for large n is out of scope.
#include "curve_routes.h"

namespace sd {

constexpr int TVD_SLICES = 16;                                     // row slices of the folds
constexpr int TVD_REC = 4;                                         // SD (int64 bits), SS, SN, SW
constexpr int TVD_STRIP = 128, TVD_STRIP_LOG = 7;                  // positions per strip
constexpr int TVD_PW_THREADS = 256, TVD_PW_TILE = 1024;            // pairwise: targets a block, curves a tile

struct TvdAcc {
    i64 sd;
    double ss, sn, sw;
};

__device__ __forceinline__ void tvd_point(i64 n, i64 a_t, TvdAcc &acc) { acc.sd += a_t * (n - a_t); }

// step t >= 1 of a target: a_s, a_t in [1, n], c = c_t, ys and yt its own values
__device__ __forceinline__ void tvd_step(i64 n, i64 a_s, i64 a_t, i64 c, double ys, double yt, TvdAcc &acc) {
    const double d = fabs(yt - ys);
    const i64 ps = a_s * (n - a_s), pt = a_t * (n - a_t);
    double S = 1.0;
    if (ps != 0 && pt != 0) {
        const double e = (double)(n * c - a_s * a_t);
        S = (e * e) / ((double)ps * (double)pt);
    }
    acc.ss += S;
    acc.sn += d * S;
    acc.sw += d;
}

__device__ __forceinline__ void tvd_load(const double *__restrict__ p, int first, TvdAcc &acc) {
    acc.sd = 0;
    acc.ss = acc.sn = acc.sw = 0.0;
    if (!first) {
        acc.sd = (i64)__double_as_longlong(p[0]);
        acc.ss = p[1];
        acc.sn = p[2];
        acc.sw = p[3];
    }
}

__device__ __forceinline__ void tvd_store(double *__restrict__ p, const TvdAcc &acc) {
    p[0] = __longlong_as_double((long long)acc.sd);
    p[1] = acc.ss;
    p[2] = acc.sn;
    p[3] = acc.sw;
}

// ---------------------------------------------------------------------------------------------- the dominance kernel
static inline int tvd_strips(i64 n) { return (int)((n + TVD_STRIP - 1) >> TVD_STRIP_LOG); }
static inline size_t tvd_dominance_lds(i64 n) {
    const size_t nb = (size_t)tvd_strips(n), sp = nb | 1;
    const size_t cells = (nb * sp + 1) & ~(size_t)1;                // H is zeroed and counted in u32 words
    return (2 * TVD_STRIP * sp + cells) * 2;
}

constexpr u64 TVD_FLAGS = 0x8000800080008000ull, TVD_FIELDS = 0x0001000100010001ull;   // bit 15 / bit 0 of the four u16 fields

// where entry k of strip b = p >> 7, k = p & 127, lies (in u16): four consecutive entries of a strip share an 8-byte word,
// the words of one group of four across the strips are consecutive
__device__ __forceinline__ u32 tvd_entry(u32 p, int SP) {
    const u32 k = p & (TVD_STRIP - 1);
    return (((k >> 2) * (u32)SP + (p >> TVD_STRIP_LOG)) << 2) | (k & 3);
}

__device__ __forceinline__ u32 tvd_wave_scan(u32 v, int lane) {    // inclusive
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// C[tl][i] = c_i - 1 of the row pair (tl - 1, tl), tl = blockIdx.x + first_local, rows local to the image; row -1 is carry
template <int EPT>
__global__ __launch_bounds__(1024) void tvd_dominance_kernel(const u32 *__restrict__ img, const u32 *__restrict__ carry, int n,
                                                             int first_local, unsigned short *__restrict__ C) {
    extern __shared__ u64 tvd_lds64[];                              // the strips are read in 8-byte words
    u32 *tvd_lds = reinterpret_cast<u32 *>(tvd_lds64);
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, waves = nthr >> 6;
    const i64 tl = (i64)blockIdx.x + first_local;
    const u32 *rt = img + tl * n, *rs = tl > 0 ? img + (tl - 1) * n : carry;
    const int nb = (n + TVD_STRIP - 1) >> TVD_STRIP_LOG, SP = nb | 1;
    unsigned short *TX = reinterpret_cast<unsigned short *>(tvd_lds), *TY = TX + TVD_STRIP * SP, *H = TY + TVD_STRIP * SP;
    u32 *cnt = tvd_lds;                                             // n counters under TX and TY (n <= 128 SP)
    const int strip_words = TVD_STRIP * SP, cell_words = (nb * SP + 1) >> 1;   // TX and TY together; H

    u32 qx[EPT], qy[EPT];                                           // position | last position of the run of ties << 16
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const u32 *row = pass ? rt : rs;
        for (int i = tid; i < n; i += nthr) cnt[i] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int i = tid + k * nthr;
            u32 q = 0;
            if (i < n) {
                const u32 w = row[i], B = w & 0xFFFFu, A = w >> 16;
                u32 pos = B + atomicAdd(&cnt[B < (u32)n ? B : 0], 1u);
                pos = pos < (u32)n ? pos : (u32)n - 1;              // (only a row with NaN, outside the contract, gets here)
                const u32 last = A < (u32)n ? (u32)n - 1 - A : 0;
                q = pos | last << 16;
            }
            if (pass) qy[k] = q;
            else qx[k] = q;
        }
        __syncthreads();
    }
    for (int i = tid; i < strip_words; i += nthr) tvd_lds[i] = 0x7FFF7FFFu;   // a missing entry of the last strip is in no count
    u32 *Hw = reinterpret_cast<u32 *>(H);
    for (int i = tid; i < cell_words; i += nthr) Hw[i] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int i = tid + k * nthr;
        if (i < n) {
            const u32 xp = qx[k] & 0xFFFFu, yp = qy[k] & 0xFFFFu;
            TX[tvd_entry(xp, SP)] = (unsigned short)yp;
            TY[tvd_entry(yp, SP)] = (unsigned short)xp;
            const u32 h = (xp >> TVD_STRIP_LOG) * SP + (yp >> TVD_STRIP_LOG);
            atomicAdd(&Hw[h >> 1], (h & 1) ? 0x10000u : 1u);        // a cell holds at most 128: no carry into its neighbour
        }
    }
    __syncthreads();
    // inclusive prefix sums of H: along by, then along bx; a lane holds two cells; the largest sum is n <= 16 384
    for (int dir = 0; dir < 2; ++dir) {
        for (int r = wave; r < nb; r += waves) {
            const int i0 = dir ? (2 * lane) * SP + r : r * SP + 2 * lane, i1 = dir ? i0 + SP : i0 + 1;
            const bool in0 = 2 * lane < nb, in1 = 2 * lane + 1 < nb;
            const u32 c0 = in0 ? H[i0] : 0u, c1 = in1 ? H[i1] : 0u;
            const u32 incl = tvd_wave_scan(c0 + c1, lane);
            if (in0) H[i0] = (unsigned short)(incl - c1);
            if (in1) H[i1] = (unsigned short)incl;
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int i = tid + k * nthr;
        if (i < n) {
            const u32 mx = qx[k] >> 16, my = qy[k] >> 16;
            const u32 qbx = mx >> TVD_STRIP_LOG, kx = mx & (TVD_STRIP - 1), qby = my >> TVD_STRIP_LOG, ky = my & (TVD_STRIP - 1);
            // Four entries a read, counted in their 16-bit fields at once.  Entries are at most 0x7FFF, so with a threshold
            // h <= 0x3FFF the field 0x8000 + h - v borrows from no neighbour and has bit 15 set iff v <= h; the y-strip's
            // "xp < 128 qbx" is h = 128 qbx - 1, which is -1 (no entry) for qbx = 0: the field 0x7FFF + 128 qbx - v.
            const u64 tx = TVD_FLAGS | (u64)my * TVD_FIELDS, ty = (u64)(0x7FFFu + (qbx << TVD_STRIP_LOG)) * TVD_FIELDS;
            const u64 *sx = reinterpret_cast<const u64 *>(TX) + qbx, *sy = reinterpret_cast<const u64 *>(TY) + qby;
            u32 c = (qbx && qby) ? H[(qbx - 1) * SP + qby - 1] : 0u;
            // the groups below the one that holds entry kx (ky) count whole, those above not at all ...
            const u32 gx = kx >> 2, gy = ky >> 2;
#pragma unroll 8
            for (u32 g = 0; g < (u32)TVD_STRIP / 4; ++g) {
                const u64 mx_g = g < gx ? TVD_FLAGS : 0ull, my_g = g < gy ? TVD_FLAGS : 0ull;
                c += (u32)__popcll((tx - sx[g * SP]) & mx_g) + (u32)__popcll((ty - sy[g * SP]) & my_g);
            }
            // ... and that group up to the entry: 16 bits of flags dropped for each entry past it
            c += (u32)__popcll((tx - sx[gx * SP]) & (TVD_FLAGS >> (16 * (3 - (kx & 3))))) +
                 (u32)__popcll((ty - sy[gy * SP]) & (TVD_FLAGS >> (16 * (3 - (ky & 3)))));
            C[tl * n + i] = (unsigned short)(c - 1);
        }
    }
}

// ---------------------------------------------------------------------------------------------- the folds
// part[q][y] (=, or +=) the record of target q over the image rows r with (row0 + r) % 16 == y
__global__ __launch_bounds__(1024) void tvd_fold_kernel(const u32 *__restrict__ img, const u32 *__restrict__ carry,
                                                        const unsigned short *__restrict__ C, const double *__restrict__ Y,
                                                        i64 row0, i64 rows, i64 n, const i64 *__restrict__ targets, i64 m,
                                                        double *__restrict__ part, u32 *__restrict__ counts) {
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const i64 q = (i64)blockIdx.x * 64 + x;
    if (q >= m) return;
    const i64 i = targets ? targets[q] : q;
    TvdAcc acc;
    double *rec = part + (q * TVD_SLICES + y) * TVD_REC;
    tvd_load(rec, row0 == 0, acc);
    i64 r = (y - row0 % TVD_SLICES + TVD_SLICES) % TVD_SLICES;
#pragma unroll 2
    for (; r < rows; r += TVD_SLICES) {
        const i64 t = row0 + r;
        const i64 a_t = n - (i64)(img[r * n + i] >> 16);
        tvd_point(n, a_t, acc);
        if (t > 0) {
            const u32 ws = r > 0 ? img[(r - 1) * n + i] : carry[i];
            const i64 c = (i64)C[r * n + i] + 1;
            tvd_step(n, n - (i64)(ws >> 16), a_t, c, Y[(t - 1) * n + i], Y[t * n + i], acc);
            if (counts) counts[(t - 1) * m + q] = (u32)c;
        }
    }
    tvd_store(rec, acc);
}

// part[q][y] = the record of target q over the rows t with t % 16 == y, by comparison with every curve
__global__ __launch_bounds__(TVD_PW_THREADS) void tvd_pairwise_kernel(const double *__restrict__ Y, i64 T, i64 n,
                                                                      const i64 *__restrict__ targets, i64 m,
                                                                      double *__restrict__ part, u32 *__restrict__ counts) {
    __shared__ double ts[TVD_PW_TILE], tt[TVD_PW_TILE];
    const int y = blockIdx.y;
    const i64 q = (i64)blockIdx.x * TVD_PW_THREADS + threadIdx.x;
    const bool live = q < m;
    const i64 i = live ? (targets ? targets[q] : q) : 0;
    TvdAcc acc;
    tvd_load(nullptr, 1, acc);
    for (i64 t = y; t < T; t += TVD_SLICES) {
        const double yt = Y[t * n + i], ys = t > 0 ? Y[(t - 1) * n + i] : 0.0;
        u32 a_s = 0, a_t = 0, c = 0;
        for (i64 j0 = 0; j0 < n; j0 += TVD_PW_TILE) {
            const int len = (int)(n - j0 < TVD_PW_TILE ? n - j0 : TVD_PW_TILE);
            __syncthreads();
            for (int j = threadIdx.x; j < len; j += TVD_PW_THREADS) {
                tt[j] = Y[t * n + j0 + j];
                if (t > 0) ts[j] = Y[(t - 1) * n + j0 + j];
            }
            __syncthreads();
            if (t > 0) {
#pragma unroll 4
                for (int j = 0; j < len; ++j) {
                    const bool bs = ts[j] <= ys, bt = tt[j] <= yt;
                    a_s += bs;
                    a_t += bt;
                    c += bs & bt;
                }
            } else {
#pragma unroll 4
                for (int j = 0; j < len; ++j) a_t += tt[j] <= yt;
            }
        }
        if (live) {
            tvd_point(n, (i64)a_t, acc);
            if (t > 0) {
                tvd_step(n, (i64)a_s, (i64)a_t, (i64)c, ys, yt, acc);
                if (counts) counts[(t - 1) * m + q] = c;
            }
        }
    }
    if (live) tvd_store(part + (q * TVD_SLICES + y) * TVD_REC, acc);
}

// the 16 slices of a target, in slice order
__global__ __launch_bounds__(256) void tvd_finish_kernel(const double *__restrict__ part, i64 m, i64 *__restrict__ sd_sum,
                                                         double *__restrict__ shape) {
    const i64 q = (i64)blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    i64 sd = 0;
    double ss = 0.0, sn = 0.0, sw = 0.0;
    for (int y = 0; y < TVD_SLICES; ++y) {
        const double *p = part + (q * TVD_SLICES + y) * TVD_REC;
        sd += (i64)__double_as_longlong(p[0]);
        ss += p[1];
        sn += p[2];
        sw += p[3];
    }
    sd_sum[q] = sd;
    shape[q * 3 + 0] = ss;
    shape[q * 3 + 1] = sn;
    shape[q * 3 + 2] = sw;
}

// ---------------------------------------------------------------------------------------------- workspaces
// behind the time-major copy: the slices' records, then on the LDS route the carried row, C and stage 1's batch
static inline size_t tvd_part_bytes(i64 m) { return align_up((size_t)m * TVD_SLICES * TVD_REC * 8, 256); }
// Stage 1 sized for r rows takes as many rows as that size holds -- r, or more where the padding of a small image leaves
// room -- and C is sized for what it takes: both from the one PairImagePlan.  By bytes, r is the most whose C and stage 1
// fit (their sum does not fall as r grows); the recommended size is for the most rows stage 1 takes in a batch.
TvdPlan tvd_plan(i64 T, i64 n, i64 m, int route, PlanSize size) {
    TvdPlan p{{route, 0, 0}, 0, tvd_part_bytes(m)};
    if (route != 1) {
        p.rows = size.rows || size.bytes >= p.bytes ? T : 0;
        return p;
    }
    const size_t fixed = p.bytes + align_up((size_t)n * 4, 256);
    auto batch = [&](i64 r) {
        const PairImagePlan s1 = pair_image_plan(T, n, 1, PlanSize::of_rows(r));
        return TvdPlan{s1, s1.rows, fixed + align_up((size_t)s1.rows * n * 2, 256) + s1.bytes};
    };
    i64 lo = 1, hi = pair_image_plan(T, n, 1, PlanSize::of_rows(T)).rows;
    if (size.rows) return batch(size.rows < hi ? size.rows : hi);
    if (size.bytes < batch(1).bytes) return p;
    while (lo < hi) {
        const i64 mid = (lo + hi + 1) >> 1;
        if (batch(mid).bytes <= size.bytes) lo = mid;
        else hi = mid - 1;
    }
    return batch(lo);
}

// ---------------------------------------------------------------------------------------------- host
struct TvdImageFold final : RankImageConsumer {
    const double *Y;
    i64 T, n, m;
    const i64 *targets;
    u32 *carry;
    unsigned short *C;
    double *part;
    u32 *counts;
    int image32(const u32 *img, i64 row0, i64 rows, hipStream_t s) override {
        const int first_local = row0 == 0 ? 1 : 0;
        const i64 pairs = rows - first_local;
        if (pairs > 0) {
            const size_t lds = tvd_dominance_lds(n);
            const bool small = n <= 4096;
            const int ept = small ? 4 : 16;
            i64 threads = align_up((size_t)((n + ept - 1) / ept), 64);
            threads = threads > 1024 ? 1024 : threads;
            const void *kf = small ? (const void *)tvd_dominance_kernel<4> : (const void *)tvd_dominance_kernel<16>;
            SD_HIP(hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            if (small)
                hipLaunchKernelGGL(tvd_dominance_kernel<4>, dim3((unsigned)pairs), dim3((unsigned)threads), lds, s, img, carry, (int)n,
                                   first_local, C);
            else
                hipLaunchKernelGGL(tvd_dominance_kernel<16>, dim3((unsigned)pairs), dim3((unsigned)threads), lds, s, img, carry, (int)n,
                                   first_local, C);
            SD_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(tvd_fold_kernel, dim3((unsigned)((m + 63) / 64)), dim3(1024), 0, s, img, carry, C, Y, row0, rows, n, targets,
                           m, part, counts);
        SD_HIP(hipGetLastError());
        if (row0 + rows < T)
            SD_HIP(hipMemcpyAsync(carry, img + (rows - 1) * n, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        return SD_OK;
    }
    int image64(const u64 *, i64, i64, hipStream_t) override { return fail(SD_ERR_INVALID, "K17 takes the u32 pair image"); }
};

int launch_tvd_sums(const double *Y, i64 T, i64 n, const i64 *targets, i64 m, int route, i64 *sd_sum, double *shape,
                    u32 *counts, void *ws, size_t ws_bytes, hipStream_t s) {
    const TvdPlan plan = tvd_plan(T, n, m, route, PlanSize::of_bytes(ws_bytes));
    Carver cv(ws, ws_bytes);
    double *part = (double *)cv.take((size_t)m * TVD_SLICES * TVD_REC * 8);
    if (!part || plan.rows < 1) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_tvd_min_workspace_bytes)");
    if (route == 1) {
        u32 *carry = (u32 *)cv.take((size_t)n * 4);
        unsigned short *C = (unsigned short *)cv.take((size_t)plan.rows * n * 2);
        void *w1 = cv.take(plan.stage1.bytes);
        if (!carry || !C || !w1) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_tvd_min_workspace_bytes)");
        TvdImageFold fold;
        fold.Y = Y, fold.T = T, fold.n = n, fold.m = m, fold.targets = targets, fold.carry = carry, fold.C = C;
        fold.part = part, fold.counts = counts;
        int rc = launch_rank_pair_images(plan.stage1, Y, T, n, fold, w1, s);
        if (rc) return rc;
    } else {
        const dim3 grid((unsigned)((m + TVD_PW_THREADS - 1) / TVD_PW_THREADS), TVD_SLICES);
        hipLaunchKernelGGL(tvd_pairwise_kernel, grid, dim3(TVD_PW_THREADS), 0, s, Y, T, n, targets, m, part, counts);
        SD_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(tvd_finish_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, part, m, sd_sum, shape);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

}  // namespace sd
