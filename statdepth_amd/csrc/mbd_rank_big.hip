// mbd_rank_big.hip -- K1+K2 rank formulation for rows that do not fit one CU's LDS
// (16 384 < n < 2^31 curves; BASELINE.json config 3, the north-star stretch case, and every multi-GPU run).
//
// Same integers as the other K1+K2 kernels (reference loops _functional.py:246-251, _containment.py:75-77).
// Per row the ranks B (others strictly below) and A (strictly above) of every curve are written as a pair image
// (AB2, rank_big_common.h); fold_ab2_image (mbd_rank_fold.hip) folds C(v,j) - C(A,j) - C(B,j) over the rows.
//
// A row is sample-partitioned into value buckets, so that no rank needs another bucket's keys.  Four launches per batch:
//   S3 bucket_setup_kernel      one workgroup per row sorts a strided sample in LDS (rank_sort.h) and publishes, per row:
//                               NB + 1 splitters (NB ~ n / 5 500 interior buckets of capacity 8 192; the sample's extremes
//                               are splitters too: the keys beyond them form two small end buckets), a LOOK-UP TABLE over
//                               TB_C cells of the monotone map c(x) = trunc((x - lo) * scale) holding, per cell, the number
//                               of splitters in earlier cells and up to this cell; a "tied" flag when the sorted sample has
//                               two equal neighbours; and the zeroing of the row's counters (no memset launch).
//   P3 bucket_partition3_kernel bucket(x) = number of splitters < x (equal values always land together), from the table: a
//                               compare is needed only in cells that a splitter cuts.  Records are 8 bytes: the curve index
//                               and a 32-bit IMAGE q of the key, monotone inside its bucket (interior buckets: linear
//                               between the two splitters; end buckets: a float-like code of the distance to the splitter
//                               in representable doubles) -- equal keys have equal images, different keys almost always
//                               different ones.  Rows flagged "tied" keep 12-byte fp64 records (their images would collide
//                               en masse).  NaNs never enter a bucket: they are counted and marked in the pair image here.
//   A3 bucket_rank32_kernel     one workgroup per (row, bucket) ranks WITHOUT a sort on the 32-bit images: a monotone map
//                               onto fine buckets (LDS histogram), prefix sum, scatter, and every key counts the members of
//                               its own fine bucket below itself: 4-byte LDS slots, integer compares.  A key whose image
//                               equals another member's settles the order of those members with their fp64 values
//                               (gathered from the matrix through the records' curve indices): exact whatever the data,
//                               cheap because it is rare on continuous data.  Tied rows run the fp64 form of the same
//                               ranking (bucket_rank_item, rank_big_common.h) inside this kernel.  A bucket with a crowded
//                               fine bucket is flagged (gate word 0).
//   big_fallback_kernel         behind two gate words, so that with nothing flagged every workgroup reads them and leaves:
//                               the flagged buckets (sort of the plain values + binary search inside the bucket, exact for
//                               ties), then -- for the rows whose partition overflowed a bucket (a quarter of the row tied
//                               on one value, say) -- the chunked route: the row is cut into chunks of 16 384 keys in curve
//                               order, every chunk is sorted, the (CU-resident) grid meets at a counter, and every sorted
//                               chunk of the row streams through LDS for the lower/upper bounds of every key.
// Why the steps look like this (profiles/r02b_config3_*): a binary search over the splitters cost 91 VALU + 46 SALU per
// key; fp64 compares run at half rate on MI355X and 8-byte LDS slots lost 63 % of their cycles to bank conflicts; separate
// fall-back launches of full grids did nothing.  The generations that had those properties are kept as independent
// implementations for the parity tests in mbd_rank_big_retired.hip (cross-check library only), reached through
// retired_big_rank_batch (rank_routes.h) when a cross-check switch asks for them.
// Work per row: one streaming pass + n/5 500 bucket rankings; config 3 (10^5 x 256) on one MI355X: see DESIGN.md.
#include <stdlib.h>

#include <atomic>

#include "rank_big_common.h"
#include "rank_routes.h"

namespace sd {

constexpr int BK_FILL = 5500;                  // target mean fill
static inline int bucket_count(i64 n) {
    // mean fill 5 500 of 8 192; past ~300 buckets even the 16 384-value sample leaves < 50 samples per bucket and the
    // fills scatter too much: aim lower
    const i64 fill = n > 1600000 ? (i64)BK_FILL * 3800 / 5500 : BK_FILL;
    i64 nb = (n + fill - 1) / fill;
    if (nb < 2) nb = 2;
    return (int)nb;
}

// =====================================================================================================
// S3 / P3 / A3
// =====================================================================================================
constexpr int TB_C = 2048;                                             // cells of the partition's look-up table
constexpr int S3_RUN = 4;                                              // neighbours per sample position (bucket_setup_kernel)
constexpr u32 Q_MAX = 0xFFFFFFFEu;                                     // largest image (0xFFFFFFFF = "no key" in LDS)

__device__ __forceinline__ u32 tb_cell(double x, double lo, double scale) {
    double u = (x - lo) * scale;                                       // monotone in x for any lo and any scale >= 0
    u = u > 0.0 ? u : 0.0;                                             // NaN (inf * 0) -> 0
    u = u < (double)(TB_C - 1) ? u : (double)(TB_C - 1);
    return (u32)u;
}
// order-preserving 64-bit pattern of a double (zeros canonicalised by the caller: x + 0.0)
__device__ __forceinline__ u64 q_ord(double x) {
    const u64 b = (u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// monotone 32-bit code of a 64-bit distance: exact below 2^27, then 26 mantissa bits under a 6-bit length field
__device__ __forceinline__ u32 q_code(u64 d) {
    if (d < (1ull << 27)) return (u32)d;
    const int e = 64 - __builtin_clzll(d);                              // 28 .. 64
    const u32 mant = (u32)(d >> (e - 27));                              // [2^26, 2^27)
    return ((u32)(e - 26) << 26) + (mant - (1u << 26));
}

template <bool MAX>
__device__ __forceinline__ u32 rb_mmu(u32 a, u32 b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); }
template <bool MAX>
__device__ __forceinline__ u32 rb_wave_allreduce_u32(u32 v) {
    v = rb_mmu<MAX>(v, (u32)__builtin_amdgcn_mov_dpp((int)v, 0x121, 0xF, 0xF, false));
    v = rb_mmu<MAX>(v, (u32)__builtin_amdgcn_mov_dpp((int)v, 0x122, 0xF, 0xF, false));
    v = rb_mmu<MAX>(v, (u32)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, false));
    v = rb_mmu<MAX>(v, (u32)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, false));
    u32 r = rb_readlane(v, 0);
    r = rb_mmu<MAX>(r, rb_readlane(v, 16));
    r = rb_mmu<MAX>(r, rb_readlane(v, 32));
    r = rb_mmu<MAX>(r, rb_readlane(v, 48));
    return r;
}

// S3: grid = rows.  NB = interior buckets; NBT = NB + 2 buckets and NS = NB + 1 splitters per row.
constexpr int FB_MEET_WORDS_S3 = 2 + 1024;                             // = FB_MEET_WORDS (checked where that is defined)
template <int SNT, int SE>
__global__ __launch_bounds__(SNT) void bucket_setup_kernel(const double *__restrict__ Y, i64 n, i64 row0, int NB,
                                                           double *__restrict__ spl, double *__restrict__ mk,
                                                           u32 *__restrict__ tab, double2 *__restrict__ rp,
                                                           u32 *__restrict__ rowtied, u32 *__restrict__ bcnt,
                                                           u32 *__restrict__ bflag, u32 *__restrict__ nnanrow,
                                                           u32 *__restrict__ ovf, u32 *__restrict__ nanf,
                                                           u32 *__restrict__ meet) {
    using Cfg = R2Cfg<SNT, SE>;
    constexpr int E = SE, LE = Cfg::LE, SS = SNT * SE, NWV = SNT / 64, CPT = TB_C / SNT;
    static_assert(TB_C % SNT == 0, "whole cells per thread");
    extern __shared__ double Sm[];
    __shared__ u32 s_cnt[TB_C];
    __shared__ u32 s_w[16];
    __shared__ u32 s_inf[2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const i64 rb = blockIdx.x;
    const int NBT = NB + 2, NS = NB + 1;
    const double *row = Y + (row0 + rb) * n;
    const double INF = __builtin_huge_val();
    double k[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const i64 sidx = (i64)t * E + e;
        // the sample in runs of S3_RUN neighbours (32 bytes: one memory request fetches four keys, S3 22.3 -> 15.1 us and
        // 33 -> 9 MB at config 3).  Runs of 8 / 16 gain 1 / 2 us more and leave fewer independent positions when
        // neighbouring curves resemble each other.
        i64 sp = ((sidx / S3_RUN) * n) / (SS / S3_RUN) + (sidx % S3_RUN);
        sp = sp < n ? sp : n - 1;
        double v = row[sp];
        k[e] = (v == v) ? v : INF;
    }
    for (int c = t; c < TB_C; c += SNT) s_cnt[c] = 0;
    if (t < 2) s_inf[t] = 0;
    // the row's counters (the partition adds to them): zeroed here, no memset launch
    for (int b = t; b < NBT; b += SNT) {
        bcnt[rb * NBT + b] = 0;
        bflag[rb * NBT + b] = 0;
    }
    if (t == 0) { nnanrow[rb] = 0; ovf[rb] = 0; nanf[rb] = 0; }
    if (rb == 0)                                                       // the batch's meeting words (big_fallback_kernel)
        for (int c = t; c < FB_MEET_WORDS_S3; c += SNT) meet[c] = 0;
    R2Sorter<SNT, SE>::sort(k, Sm, t, SS, true, INF);
    double *Sw = Sm + r2_base<0, LE>(t);
#pragma unroll
    for (int e = 0; e < E; ++e) Sw[r2_off<0, LE>(e)] = k[e];
    u32 cpos = 0, cneg = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        cpos += (k[e] == INF) ? 1u : 0u;
        cneg += (k[e] == -INF) ? 1u : 0u;
    }
    if (cpos) atomicAdd(&s_inf[0], cpos);
    if (cneg) atomicAdd(&s_inf[1], cneg);
    __syncthreads();
    // two equal neighbours in the sorted sample: the row is tie-heavy (or holds several NaN / infinities)
    bool tie = false;
#pragma unroll
    for (int e = 0; e + 1 < E; ++e) tie |= k[e] == k[e + 1];
    if (t + 1 < SNT) tie |= k[E - 1] == Sm[r2_phys<LE>((t + 1) * E)];
    const int anytie = __syncthreads_or(tie);
    // cell map over the finite part of the sample
    const int ilo = (int)(s_inf[1] < (u32)(SS - 1) ? s_inf[1] : (u32)(SS - 1));
    const int ihi = SS - 1 - (int)(s_inf[0] < (u32)(SS - 1) ? s_inf[0] : (u32)(SS - 1));
    const double lo = Sm[r2_phys<LE>(ilo)], hi = Sm[r2_phys<LE>(ihi)];
    double scale = (double)TB_C / (hi - lo);
    if (!(scale > 0.0 && scale < INF)) scale = 0.0;                     // degenerate range: one cell, plain search
    for (int j = t; j < NS; j += SNT) {
        const int pos = (j == 0) ? 0 : (j == NS - 1) ? SS - 1 : (int)(((i64)j * SS) / NB);
        const double sj = Sm[r2_phys<LE>(pos)] + 0.0;                   // -0 -> +0
        spl[rb * NS + j] = sj;
        atomicAdd(&s_cnt[tb_cell(sj, lo, scale)], 1u);
        if (j >= 1) {                                                   // interior bucket j = (s_{j-1}, s_j]
            const int pp = (j - 1 == 0) ? 0 : (int)(((i64)(j - 1) * SS) / NB);
            const double sp = Sm[r2_phys<LE>(pp)] + 0.0;
            double m = (double)Q_MAX / (sj - sp);
            // The outermost interior buckets reach from the first / last quantile splitter to the sample's extreme: under heavy
            // tails nearly all of their keys sit at the inner end and a linear image crowds them into a few of A3's fine buckets
            // (Cauchy rows: 81 keys in the first, above its 63 -- the value bucket went to the search kernel, 120 us at config
            // 3's size).  Where the sample's median inside such a bucket lies in the inner eighth of its range the bucket takes
            // the float-like code of the distance to its inner splitter, like the end buckets beyond it (mk = 0 says so).
            if (j == 1 && NS >= 3) {
                const double med = Sm[r2_phys<LE>(pos / 2)];
                if ((sj - med) * 8.0 < (sj - sp)) m = 0.0;
            } else if (j == NS - 1 && NS >= 3) {
                const double med = Sm[r2_phys<LE>((pp + pos) / 2)];
                if ((med - sp) * 8.0 < (sj - sp)) m = 0.0;
            }
            mk[rb * NBT + j] = m;
        }
    }
    if (t == 0) {
        mk[rb * NBT] = 0.0;
        mk[rb * NBT + NBT - 1] = 0.0;
        rp[rb] = make_double2(lo, scale);
        rowtied[rb] = anytie ? 1u : 0u;
    }
    __syncthreads();
    // per cell: splitters in earlier cells | splitters up to and including this cell
    u32 c[CPT], run = 0;
#pragma unroll
    for (int q = 0; q < CPT; ++q) { c[q] = s_cnt[t * CPT + q]; run += c[q]; }
    const u32 incl = rb_wave_incl_scan(run);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    u32 base = incl - run;
    for (int w = 0; w < wave; ++w) base += s_w[w];
    (void)NWV;
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
        tab[rb * TB_C + t * CPT + q] = base | ((base + c[q]) << 16);
        base += c[q];
    }
}

// P3: grid = (ceil(n / 3072), rows), 512 threads x 6 keys
// 6 keys per thread (8: 4 096 keys per block and three workgroups per CU -- + 2 ... 3 % at every size measured)
constexpr int P3_NT = 512, P3_E = 6, P3_C = P3_NT * P3_E;
static inline size_t p3_lds_bytes(int NBT) {
    return (size_t)P3_C * 8 + (size_t)(2 * NBT + 2) * 8 + (size_t)TB_C * 4 + (size_t)(3 * NBT + 4 + P3_NT / 64) * 4 + (size_t)P3_C * 2 + 64;
}
__global__ __launch_bounds__(P3_NT) void bucket_partition3_kernel(const double *__restrict__ Y, i64 n, i64 row0, int NBT,
                                                                  const double *__restrict__ spl,
                                                                  const double *__restrict__ mk,
                                                                  const u32 *__restrict__ tab,
                                                                  const double2 *__restrict__ rp,
                                                                  const u32 *__restrict__ rowtied,
                                                                  u32 *__restrict__ bcnt, u32 *__restrict__ nnanrow,
                                                                  u32 *__restrict__ ovf, u64 *__restrict__ rec,
                                                                  u32 *__restrict__ bidx, u32 *__restrict__ gate,
                                                                  u32 epoch, AB2 ab) {
    // One block of 3 072 curves of one row per workgroup, four workgroups per CU up to ~30 value buckets (40 KB of LDS; with
    // 4 096 curves: three).  Keys per thread 4 / 5 / 6 / 7 / 8 / 10 at config 3: 0.272 / 0.265 / 0.267 / 0.278 / 0.274 / 0.293 ms
    // (profiles/r04_p3_keys_per_thread.txt).  (Measured and dropped: 4 consecutive
    // blocks per workgroup with the next block's keys prefetched and the row's table loaded once -- 95 VGPRs, two workgroups
    // per CU, 128 us against 111 us at config 3: the third resident workgroup hides more latency than the prefetch.)
    extern __shared__ double Sm3[];
    const int NS = NBT - 1;
    u64 *stage = reinterpret_cast<u64 *>(Sm3);                         // [P3_C] records in bucket order
    double *s_spl = Sm3 + P3_C;                                        // [NS]
    double *s_mk = s_spl + NBT;                                        // [NBT]
    u32 *s_tab = reinterpret_cast<u32 *>(s_mk + NBT + 2);              // [TB_C]
    u32 *s_hist = s_tab + TB_C;                                        // [NBT]
    u32 *s_gbase = s_hist + NBT;                                       // [NBT]
    u32 *s_lbase = s_gbase + NBT;                                      // [NBT + 1]
    u32 *s_wtot = s_lbase + NBT + 2;                                   // [P3_NT / 64]
    unsigned short *sbk = reinterpret_cast<unsigned short *>(s_wtot + P3_NT / 64 + 1);   // [P3_C]
    const i64 rb = blockIdx.y;
    const double *row = Y + (row0 + rb) * n;
    const i64 base = (i64)blockIdx.x * P3_C;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double x[P3_E];
#pragma unroll
    for (int e = 0; e < P3_E; ++e) {
        const i64 i = base + t + e * P3_NT;
        x[e] = (i < n) ? row[i] : 0.0;
    }
    for (int c = t; c < TB_C; c += P3_NT) s_tab[c] = tab[rb * TB_C + c];
    for (int b = t; b < NBT; b += P3_NT) {
        if (b < NS) s_spl[b] = spl[rb * NS + b];
        s_mk[b] = mk[rb * NBT + b];
        s_hist[b] = 0;
    }
    const double2 prm = rp[rb];
    const bool tied = rowtied[rb] != 0;                                // block-uniform
    const int per = (NBT + P3_NT - 1) / P3_NT;                         // buckets per thread in the prefix phase (<= 3)
    u32 mynan = 0;
    bool over = false;
    __syncthreads();
    {
        u32 bk[P3_E], off[P3_E], q[P3_E];
#pragma unroll
        for (int e = 0; e < P3_E; ++e) {
            const i64 i = base + t + e * P3_NT;
            bk[e] = 0xFFFFFFFFu;
            off[e] = 0;
            q[e] = 0;
            if (i < n) {
                const double xv = x[e];
                if (xv == xv) {
                    const u32 tb = s_tab[tb_cell(xv, prm.x, prm.y)];
                    int a = (int)(tb & 0xFFFFu), b = (int)(tb >> 16);   // bucket = number of splitters < x, in [a, b]
                    while (a < b) {
                        const int mid = (a + b) >> 1;
                        if (s_spl[mid] < xv) a = mid + 1;
                        else b = mid;
                    }
                    bk[e] = (u32)a;
                    {
                        // curves ordered by level put a whole wave's keys into one bucket: 64 lanes on one counter are 64
                        // serialised LDS atomics (P3 117 -> 168 us on such data).  One atomic for the wave then, the lanes
                        // take their slots in lane order; any other wave as before.
                        const u64 act = __ballot(1);
                        const u32 a0 = (u32)__builtin_amdgcn_readfirstlane(a);
                        if (__ballot((u32)a == a0) == act) {
                            const int leader = __ffsll((long long)act) - 1;
                            u32 old = 0;
                            if (lane == leader) old = atomicAdd(&s_hist[a0], (u32)__popcll(act));
                            old = rb_readlane(old, leader);
                            off[e] = old + __builtin_amdgcn_mbcnt_hi((u32)(act >> 32), __builtin_amdgcn_mbcnt_lo((u32)act, 0u));
                        } else {
                            off[e] = atomicAdd(&s_hist[a], 1u);
                        }
                    }
                    if (!tied) {
                        const double xc = xv + 0.0;
                        u32 qq;
                        if (s_mk[a] == 0.0 && a <= 1) {                 // below the sample / a skewed first interior bucket (S3)
                            const u32 cd = q_code(q_ord(s_spl[a]) - q_ord(xc));
                            qq = Q_MAX - (cd < Q_MAX ? cd : Q_MAX);
                        } else if (s_mk[a] == 0.0) {                    // above the sample / a skewed last interior bucket / no width
                            const u32 cd = q_code(q_ord(xc) - q_ord(s_spl[a - 1]));
                            qq = cd < Q_MAX ? cd : Q_MAX;
                        } else {
                            double v = (xc - s_spl[a - 1]) * s_mk[a];
                            v = v < (double)Q_MAX ? v : (double)Q_MAX; // NaN -> Q_MAX
                            qq = (u32)v;
                        }
                        q[e] = qq;
                    }
                } else {
                    ++mynan;
                    ab_store_nan(ab, (size_t)(rb * n + i));
                }
            }
        }
        __syncthreads();                                               // B1: the block's histogram is complete
        // global base of this workgroup's run in every bucket (one returning atomic per bucket: its round trip to L2 is
        // spent under the local prefix sum and the LDS scatter, the result is only needed for the copy-out); local exclusive
        // prefix of the workgroup's counts.  Thread t owns the buckets [t * per, t * per + per), per <= 3.
        u32 gb0 = 0, gb1 = 0, gb2 = 0;
        {
            u32 run = 0;
            {
                const int b = t * per;
                if (b < NBT) { const u32 c = s_hist[b]; gb0 = c ? atomicAdd(&bcnt[rb * NBT + b], c) : 0u; run += c; }
            }
            if (per > 1) {
                const int b = t * per + 1;
                if (b < NBT) { const u32 c = s_hist[b]; gb1 = c ? atomicAdd(&bcnt[rb * NBT + b], c) : 0u; run += c; }
            }
            if (per > 2) {
                const int b = t * per + 2;
                if (b < NBT) { const u32 c = s_hist[b]; gb2 = c ? atomicAdd(&bcnt[rb * NBT + b], c) : 0u; run += c; }
            }
            const u32 incl = rb_wave_incl_scan(run);
            if (lane == 63) s_wtot[wave] = incl;
            __syncthreads();                                           // B2
            u32 o = incl - run;
            for (int w = 0; w < wave; ++w) o += s_wtot[w];
            for (int r = 0; r < per; ++r) {
                const int b = t * per + r;
                if (b < NBT) {
                    s_lbase[b] = o;
                    o += s_hist[b];
                }
            }
            if (t == P3_NT - 1) s_lbase[NBT] = o;                       // non-NaN keys of the block
        }
        __syncthreads();                                               // B3
#pragma unroll
        for (int e = 0; e < P3_E; ++e) {
            if (bk[e] != 0xFFFFFFFFu) {
                const u32 lp = s_lbase[bk[e]] + off[e];
                const u32 id = (u32)(base + t + e * P3_NT);
                stage[lp] = tied ? (u64)__double_as_longlong(x[e]) : ((u64)q[e] | ((u64)id << 32));
                sbk[lp] = (unsigned short)bk[e];
            }
        }
        if (t * per < NBT) s_gbase[t * per] = gb0;
        if (per > 1 && t * per + 1 < NBT) s_gbase[t * per + 1] = gb1;
        if (per > 2 && t * per + 2 < NBT) s_gbase[t * per + 2] = gb2;
        __syncthreads();                                               // B4
        const u32 nval = s_lbase[NBT];
        for (u32 p = t; p < nval; p += P3_NT) {
            const u32 b = sbk[p];
            const u32 g = s_gbase[b] + (p - s_lbase[b]);
            if (g < (u32)BK_C) rec[((size_t)rb * NBT + b) * BK_C + g] = stage[p];
            else over = true;
        }
        if (tied) {                                                    // fp64 records: the curve indices in a second round
            __syncthreads();
            u32 *stage32 = reinterpret_cast<u32 *>(stage);
#pragma unroll
            for (int e = 0; e < P3_E; ++e)
                if (bk[e] != 0xFFFFFFFFu) stage32[s_lbase[bk[e]] + off[e]] = (u32)(base + t + e * P3_NT);
            __syncthreads();
            for (u32 p = t; p < nval; p += P3_NT) {
                const u32 b = sbk[p];
                const u32 g = s_gbase[b] + (p - s_lbase[b]);
                if (g < (u32)BK_C) bidx[((size_t)rb * NBT + b) * BK_C + g] = stage32[p];
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) mynan += __shfl_down(mynan, o);
    if (lane == 0 && mynan) atomicAdd(&nnanrow[rb], mynan);
    if (over) { ovf[rb] = 1u; gate[1] = epoch; }                       // a gate word is "set" when it holds the batch's epoch
}

// A3: grid = 8 * NBT * ceil(rows / 8) (the XCD-aware mapping of bucket_rank_kernel), 512 threads x 16 keys
constexpr int A3_NT = 512, A3_E = BK_CE, A3_LNB = 12, A3_NBF = 1 << A3_LNB, A3_CAP = 63, A3_U = 2, A3_PAD = 32;
constexpr int A3_NW = A3_NT / 64;
static_assert(A3_NT * A3_E == BK_C, "one thread slot per key of a full value bucket");
static_assert(A3_NBF / 2 / A3_NT == 4, "one 16-byte quad of histogram words per thread");
constexpr size_t A3_HDR = 256;
constexpr size_t A3_LDS32 = A3_HDR + (size_t)(A3_NBF / 2 + 4) * 4 + (size_t)(BK_C + A3_PAD) * 4 + (size_t)(BK_C + A3_PAD) * 2;
constexpr size_t A3_LDS = A3_LDS32 > BR_LDS ? A3_LDS32 : BR_LDS;      // rows flagged "tied" run A' inside this kernel

__global__ __launch_bounds__(A3_NT) void bucket_rank32_kernel(const double *__restrict__ Y, i64 n, i64 row0, i64 rows, int NBT,
                                                              const u32 *__restrict__ bcnt,
                                                              const u32 *__restrict__ nnanrow,
                                                              const u32 *__restrict__ ovf,
                                                              const u32 *__restrict__ rowtied,
                                                              const u64 *__restrict__ rec,
                                                              const u32 *__restrict__ bidx, u32 *__restrict__ bflag,
                                                              u32 *__restrict__ gate, u32 epoch, AB2 ab) {
    constexpr int E = A3_E, NT = A3_NT, NBF = A3_NBF, NW = A3_NW, U = A3_U;
    extern __shared__ double Sm[];
    u32 *red = reinterpret_cast<u32 *>(Sm);                            // [NW][2] min / max, then [NW] earlier-bucket sums
    u32 *wtot = red + 2 * NW;                                          // [NW]
    u32 *H = reinterpret_cast<u32 *>(Sm + A3_HDR / 8);                 // NBF packed u16 counters, then bases
    u32 *S = H + NBF / 2 + 4;                                          // images in fine-bucket order + sentinels
    unsigned short *Jx = reinterpret_cast<unsigned short *>(S + BK_C + A3_PAD);   // record slot of every image
    const unsigned short *H16 = reinterpret_cast<const unsigned short *>(H);
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    // the groups of 8 rows NEWEST first: the partition wrote the last rows' records last, and those are the ones the 256 MB
    // Infinity Cache still holds when this kernel starts (- 1 % at every size measured; blockIdx order: 0.2667 / 0.9026 ms at
    // 10^5 x 256 / x 1 000, this order 0.2631 / 0.8949)
    const int w = (int)(((gridDim.x >> 3) / NBT - 1 - (blockIdx.x >> 3) / NBT) * NBT + (blockIdx.x >> 3) % NBT) * 8 + (int)(blockIdx.x & 7);
    const int b = (w >> 3) % NBT;
    const i64 rb = (i64)((w >> 3) / NBT) * 8 + (w & 7);
    if (rb >= rows) return;
    if (ovf[rb]) return;
    __builtin_amdgcn_s_setprio(2);                                    // load / histogram / scatter phases go first, the member pass of the
                                                                      // CU's other workgroup fills in (A3 146 -> 137 us at config 3)
    if (rowtied[rb]) {                                                // block-uniform: fp64 records, A' (same LDS, same grid)
        bucket_rank_item(w, n, rows, NBT, bcnt, nnanrow, ovf, rowtied, reinterpret_cast<const double *>(rec), bidx, bflag,
                         gate, epoch, ab);
        return;
    }
    const u32 *rowcnt = bcnt + rb * NBT;
    const int cnt = (int)rowcnt[b];
    if (cnt == 0) return;
    const size_t slot0 = ((size_t)rb * NBT + b) * BK_C;

    u32 q[E], id[E];
    {
        const u64 *rp = rec + slot0 + t;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const u64 r = (t + e * NT < cnt) ? rp[e * NT] : 0xFFFFFFFFull;
            q[e] = (u32)r;
            id[e] = (u32)(r >> 32);
        }
    }
    u32 gsum = 0;
    for (int k = t; k < b; k += NT) gsum += rowcnt[k];
    gsum = rb_wave_incl_scan(gsum);
    reinterpret_cast<uint4 *>(H)[t] = make_uint4(0, 0, 0, 0);
    if (t < 4) H[NBF / 2 + t] = 0;
    if (t < A3_PAD) S[cnt + t] = 0xFFFFFFFFu;
    u32 mn = 0xFFFFFFFFu, mx = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (e * NT >= cnt) break;
        mn = mn < q[e] ? mn : q[e];
        const u32 v = (t + e * NT < cnt) ? q[e] : 0u;
        mx = mx > v ? mx : v;
    }
    mn = rb_wave_allreduce_u32<false>(mn);
    mx = rb_wave_allreduce_u32<true>(mx);
    if (lane == 63) { red[2 * wave] = mn; red[2 * wave + 1] = mx; wtot[wave] = gsum; }
    __syncthreads();                                                  // barrier 1
    u32 lo, hi, gbase;
    {
        const uint2 pmm = reinterpret_cast<const uint2 *>(red)[lane & (NW - 1)];
        lo = rb_wave_allreduce_u32<false>(pmm.x);
        hi = rb_wave_allreduce_u32<true>(pmm.y);
        const u32 g = (lane < NW) ? wtot[lane] : 0u;
        gbase = rb_readlane(rb_row_incl_scan(g), 15);
    }
    const u32 nreal = (u32)n - nnanrow[rb];
    const size_t abrow = (size_t)(rb * n);
    const float fs = (float)NBF / ((float)(hi - lo) + 1.0f);
    // ---- (1) fine bucket + slot ----
    u32 bs[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (e * NT >= cnt) break;
        u32 fb = (u32)((float)(q[e] - lo) * fs);                      // monotone in q
        fb = fb < (u32)(NBF - 1) ? fb : (u32)(NBF - 1);
        fb = (t + e * NT < cnt) ? fb : (u32)(NBF + 2);                // no key: dummy counter
        const u32 sh = (fb & 1u) * 16u;
        const u32 old = atomicAdd(&H[fb >> 1], 1u << sh);
        bs[e] = fb | (((old >> sh) & 0xFFFFu) << 16);
    }
    __syncthreads();                                                  // barrier 2
    // ---- (2) exclusive prefix sum; a fine bucket above A3_CAP keys: the search kernel takes the value bucket ----
    bool anyover = false;
    {
        const uint4 hq = reinterpret_cast<const uint4 *>(H)[t];
        constexpr u32 HIM = (0xFFFFu & ~(u32)A3_CAP) * 0x10001u;
        const u32 s4 = hq.x + hq.y + hq.z + hq.w;
        const u32 ov = hq.x | hq.y | hq.z | hq.w;
        const u32 run = (s4 & 0xFFFFu) + (s4 >> 16);
        const u32 incl = rb_wave_incl_scan(run);
        const bool wover = __ballot((ov & HIM) != 0) != 0;
        if (lane == 63) wtot[wave] = incl | (wover ? 0x80000000u : 0u);
        __syncthreads();                                              // barrier 3
        const u32 wt = (lane < NW) ? wtot[lane] : 0u;
        anyover = __ballot((wt >> 31) != 0) != 0;                     // block-uniform
        const u32 wscan = rb_row_incl_scan(wt & 0x7FFFFFFFu);
        u32 base = (wave ? rb_readlane(wscan, wave - 1) : 0u) + incl - run;
        uint4 o;
        o.x = base | ((base + (hq.x & 0xFFFFu)) << 16);
        base += (hq.x & 0xFFFFu) + (hq.x >> 16);
        o.y = base | ((base + (hq.y & 0xFFFFu)) << 16);
        base += (hq.y & 0xFFFFu) + (hq.y >> 16);
        o.z = base | ((base + (hq.z & 0xFFFFu)) << 16);
        base += (hq.z & 0xFFFFu) + (hq.z >> 16);
        o.w = base | ((base + (hq.w & 0xFFFFu)) << 16);
        base += (hq.w & 0xFFFFu) + (hq.w >> 16);
        reinterpret_cast<uint4 *>(H)[t] = o;
        if (t == NT - 1) H[NBF / 2] = base;                           // = cnt
    }
    if (anyover) {                                                    // heavy ties the sample did not show
        if (t == 0) { bflag[rb * NBT + b] = 1u; gate[0] = epoch; }
        return;
    }
    __syncthreads();                                                  // barrier 4
    // ---- (3) scatter into fine-bucket order ----
    u32 bc[E];                                                        // base | count << 16; count 0: no key
    const u32 dummy = (u32)(cnt + A3_PAD - 1);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (e * NT >= cnt) break;
        const u32 fb = bs[e] & 0xFFFFu, slot = bs[e] >> 16;
        const u32 base = H16[fb], end = H16[fb + 1];
        const bool isk = fb < (u32)NBF;
        const u32 pos = isk ? base + slot : dummy;
        S[pos] = isk ? q[e] : 0xFFFFFFFFu;
        Jx[pos] = (unsigned short)(t + e * NT);
        bc[e] = isk ? (base | ((end - base) << 16)) : 0u;
    }
    __syncthreads();                                                  // barrier 5
    // ---- (4) rank inside the fine bucket, write B ----
    __builtin_amdgcn_s_setprio(0);
    const double *yrow = Y + (row0 + rb) * n;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (e * NT >= cnt) break;
        if ((e & 1) == 0) __builtin_amdgcn_sched_barrier(0);
        const u32 base = bc[e] & 0xFFFFu, fc = bc[e] >> 16;
        const u32 offq = base & 3u;
        const u32 x = q[e];
        const uint4 *Sq = reinterpret_cast<const uint4 *>(S + (base - offq));
        u32 less = 0, eq = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint4 y = Sq[u];
            less += (y.x < x) + (y.y < x) + (y.z < x) + (y.w < x);
            eq += (y.x == x) + (y.y == x) + (y.z == x) + (y.w == x);
        }
        if (fc + offq > (u32)(4 * U)) {                               // a fine bucket longer than the window
            for (u32 kk = 4 * U; kk < fc + offq; kk += 4) {
                const uint4 y = Sq[kk >> 2];
                less += (y.x < x) + (y.y < x) + (y.z < x) + (y.w < x);
                eq += (y.x == x) + (y.y == x) + (y.z == x) + (y.w == x);
            }
        }
        less -= offq;                                                 // keys in front of the base: earlier fine buckets, all smaller
        if (fc) {
            if (eq == 1u) {
                ab_store_untied(ab, abrow + id[e], gbase + base + less, nreal);
            } else {
                // another member carries the same image: the fp64 values of those members decide
                const double xv = yrow[id[e]];
                u32 lt = 0, eqv = 0;
                for (u32 m = base; m < base + fc; ++m) {
                    if (S[m] == x) {
                        const u32 im = (u32)(rec[slot0 + Jx[m]] >> 32);
                        const double yv = yrow[im];
                        lt += (yv < xv) ? 1u : 0u;
                        eqv += (yv == xv) ? 1u : 0u;
                    }
                }
                const u32 Bv = gbase + base + less + lt;
                ab_store(ab, abrow + id[e], Bv, nreal - (Bv + eqv), nreal);
            }
        }
    }
}

// The three fall-backs of a batch in ONE launch (product path): flagged value buckets (gate[0]), then the chunked route for
// the rows whose partition overflowed (gate[1]): every workgroup sorts its share of the rows' chunks, the grid meets at a
// counter, every workgroup searches its share of (row, chunk) items.  Nothing flagged: every workgroup reads the two gate
// words and leaves.
// The meeting (meet[], zeroed by S3 every batch): [0] arrivals, [1] workgroups that gave up waiting, [2 + w] who searches
// workgroup w's items.  The grid is one workgroup per CU the stream may use, so every workgroup the others wait for is
// running -- unless something the host cannot see keeps CUs from this launch (a process-wide mask, another process).  So the
// wait is bounded: a workgroup that has waited spin_limit polls announces it, looks once more, and leaves its items to the
// LAST workgroup to arrive, which exists whatever happens (nobody waits for a workgroup that has not sorted yet without
// eventually making room for it) and sweeps the claim words when anybody gave up.  A claim word changes once, by
// compare-and-swap (0 -> FB_SELF by its owner, FB_LEFT by its owner on leaving, FB_TAKEN by the last arriver): every item is
// searched exactly once.
constexpr u32 FB_SELF = 1u, FB_LEFT = 2u, FB_TAKEN = 3u;
constexpr int FB_MAXGRID = 1024;
constexpr int FB_MEET_WORDS = 2 + FB_MAXGRID;
static_assert(FB_MEET_WORDS == FB_MEET_WORDS_S3, "S3 zeroes the meeting words");
__global__ __launch_bounds__(BIG_NT) void big_fallback_kernel(const double *__restrict__ Y, i64 n, i64 row0, i64 rows, int NBT,
                                                              const u32 *__restrict__ bcnt,
                                                              const u32 *__restrict__ nnanrow,
                                                              const u32 *__restrict__ bflag,
                                                              const u32 *__restrict__ rowtied,
                                                              const double *__restrict__ bval,
                                                              const u32 *__restrict__ bidx, double *sorted, i64 sstride,
                                                              u32 *nanf, int nch, const u32 *__restrict__ ovf,
                                                              const u32 *__restrict__ gate, u32 epoch, u32 *meet,
                                                              u32 spin_limit, AB2 ab) {
    extern __shared__ double Sm[];
    __shared__ u32 s_role;                                            // 0: leave, 1: search my items, 2: ... and sweep
    const bool flagged = gate[0] == epoch, over = gate[1] == epoch;   // block-uniform
    if (!flagged && !over) return;
    if (flagged) bucket_search_items<BIG_NT, BIG_E>(Y, n, row0, rows, NBT, bcnt, nnanrow, bflag, rowtied, bval, bidx, ab, Sm);
    if (!over) return;
    __syncthreads();
    chunk_sort_items(Y, n, row0, rows, nch, sorted, sstride, nanf, ovf, Sm);
    __syncthreads();
    const u32 G = gridDim.x, me = blockIdx.x;
    auto arrived = [&]() { return __hip_atomic_load(&meet[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    if (threadIdx.x == 0) {
        __threadfence();                                              // the sorted chunks and the NaN counts, device-wide
        const u32 ticket = atomicAdd(&meet[0], 1u);
        const bool last = ticket + 1u == G;
        bool full = last;
        for (u32 spins = 0; !full && spins < spin_limit; ++spins) {
            __builtin_amdgcn_s_sleep(32);
            full = arrived() >= G;
        }
        if (!full) {                                                  // waited long enough: say so, then look once more
            atomicAdd(&meet[1], 1u);
            __threadfence();
            full = arrived() >= G;
        }
        u32 role = 0;
        if (full) role = atomicCAS(&meet[2 + me], 0u, FB_SELF) == 0u ? 1u : 0u;
        else atomicCAS(&meet[2 + me], 0u, FB_LEFT);
        if (last) role |= 2u;
        __threadfence();
        s_role = role;
    }
    __syncthreads();
    const u32 role = s_role;
    if (role & 1u) chunk_search_items(Y, n, row0, rows, sorted, sstride, nanf, nch, ovf, ab, Sm, me, G);
    if (!(role & 2u)) return;
    // the last arriver: did anybody give up?  (Whoever did said so before its last look at the arrivals, which did not
    // include this workgroup's.)
    __syncthreads();
    if (threadIdx.x == 0) s_role = __hip_atomic_load(&meet[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_role == 0u) return;
    for (u32 w = 0; w < G; ++w) {
        if (w == me) continue;
        __syncthreads();
        if (threadIdx.x == 0) {
            const u32 v = atomicCAS(&meet[2 + w], 0u, FB_TAKEN);
            s_role = (v == 0u || v == FB_LEFT) ? 1u : 0u;
        }
        __syncthreads();
        if (s_role) chunk_search_items(Y, n, row0, rows, sorted, sstride, nanf, nch, ovf, ab, Sm, w, G);
    }
}

// =====================================================================================================
// host side
// =====================================================================================================
static inline i64 big_nchunks(i64 n) { return (n + BIG_C - 1) / BIG_C; }

struct BigPlan {
    i64 nch, sstride, rpb;
    int NB, NBT;                                         // interior value buckets; NBT = NB + 2 with the two end buckets
    size_t off_ab, off_h, off_sorted, off_bval, off_bidx, off_spl, off_mk, off_tab, off_rp, off_zero, zero_bytes, total;
    // zeroed block: bcnt[rpb*NBT] | nnanrow[rpb] | ovf[rpb] | bflag[rpb*NBT] | nanrow_f[rpb] | rowtied[rpb]
    size_t z_bcnt, z_nnan, z_ovf, z_bflag, z_nanf, z_tied, z_gate, z_meet;
};

constexpr size_t BIG_SCRATCH_BYTES = (size_t)1 << 32;   // scratch per batch (big_plan)
constexpr int S3_SMALL_NB = 24;                         // up to that many value buckets: the 2 048-key sample
constexpr int S3_MID_NB = 72;                           // ... the 4 096-key sample; beyond: 16 384 keys
static BigPlan big_plan(i64 T, i64 n) {
    BigPlan p;
    p.nch = big_nchunks(n);
    p.sstride = p.nch * BIG_C;
    p.NB = bucket_count(n);
    p.NBT = p.NB + 2;
    const size_t per_row = (size_t)n * 8 + (size_t)p.sstride * 8 + (size_t)p.NBT * BK_C * 12 + (size_t)p.NBT * 32 +
                           (size_t)TB_C * 4 + 128;
    // Scratch per batch: every batch costs 40 - 45 us by itself (S3's latency in front of the partition, the kernels' tails, the
    // fold's launch; profiles/r04_experiment_rows_per_batch.txt), and 288 GB of HBM have room: 4 GiB take 10^5 curves x 1 000
    // timepoints in one batch (1.5 GiB: three).
    i64 r = (i64)(BIG_SCRATCH_BYTES / per_row);
    const i64 vb = xswitch("SD_RANK_ROWS_PER_BATCH");          // cross-check builds: several batches on small inputs
    if (vb > 0 && vb < r) r = vb;
    if (r < 1) r = 1;
    if (r > T) r = T;
    if (r > 65535) r = 65535;
    p.rpb = r;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
    p.off_ab = take((size_t)r * n * 8);
    p.off_h = take(n <= AB2_H_MAXN ? (size_t)r * n * 2 : 0);
    p.off_sorted = take((size_t)r * p.sstride * 8);
    p.off_bval = take((size_t)r * p.NBT * BK_C * 8);
    p.off_bidx = take((size_t)r * p.NBT * BK_C * 4);
    p.off_spl = take((size_t)r * p.NBT * 8);
    p.off_mk = take((size_t)r * p.NBT * 8);
    p.off_tab = take((size_t)r * TB_C * 4);
    p.off_rp = take((size_t)r * 16);
    p.off_zero = o;
    size_t z = 0;
    auto ztake = [&](size_t bytes) { size_t at = z; z = align_up(z + bytes, 256); return at; };
    p.z_bcnt = ztake((size_t)r * p.NBT * 4);
    p.z_nnan = ztake((size_t)r * 4);
    p.z_ovf = ztake((size_t)r * 4);
    p.z_bflag = ztake((size_t)r * p.NBT * 4);
    p.z_nanf = ztake((size_t)r * 4);
    p.z_tied = ztake((size_t)r * 4);
    p.z_gate = ztake(16 * 4);                                // per batch: [0] some bucket flagged, [1] some row overflowed
    p.z_meet = ztake((size_t)FB_MEET_WORDS * 4);             // the fall-back kernel's meeting
    p.zero_bytes = z;
    p.total = o + z + 256;
    return p;
}

bool mbd_rank_big_supported(i64 T, i64 n, int J) {
    (void)T;
    return n > 16384 && n < ((i64)1 << 31) && J >= 2 && J <= JMAX && big_nchunks(n) <= 1024 &&
           bucket_count(n) + 2 <= BK_MAXNB;
}

size_t mbd_rank_big_workspace_bytes(i64 T, i64 n, int J) {
    if (!mbd_rank_big_supported(T, n, J)) return 0;
    return big_plan(T, n).total + 1024;
}

// img_out != nullptr: no fold -- the B words of every (row, curve) go to img_out[T][n] (bit 31: the curve ties with another
// one at this timepoint; 0xFFFFFFFF: NaN) and the rows' NaN counts to nnan_out[T]: the strict path's rank image for n > 32 767
static int big_run(const double *Y, i64 T, i64 n, const i64 *targets, i64 tbegin, i64 m, int J, u64 *out, void *ws,
                   size_t ws_bytes, hipStream_t s, u32 *img_out, u32 *nnan_out);

int launch_mbd_rank_big(const double *Y, i64 T, i64 n, const i64 *targets, i64 tbegin, i64 m, int J,
                        u64 *out, void *ws, size_t ws_bytes, hipStream_t s) {
    return big_run(Y, T, n, targets, tbegin, m, J, out, ws, ws_bytes, s, nullptr, nullptr);
}

int launch_rank_big_image(const double *Y, i64 T, i64 n, u32 *img, u32 *nnan, void *ws, size_t ws_bytes, hipStream_t s) {
    return big_run(Y, T, n, nullptr, 0, n, 2, nullptr, ws, ws_bytes, s, img, nnan);
}

static int big_run(const double *Y, i64 T, i64 n, const i64 *targets, i64 tbegin, i64 m, int J, u64 *out, void *ws,
                   size_t ws_bytes, hipStream_t s, u32 *img_out, u32 *nnan_out) {
    if (!mbd_rank_big_supported(T, n, J)) return fail(SD_ERR_UNSUPPORTED, "large-n rank kernels cover n > 16384");
    const BigPlan p = big_plan(T, n);
    if (!ws || ws_bytes < p.total) return fail(SD_ERR_WORKSPACE, "large-n rank workspace too small");
    char *w = (char *)(((size_t)ws + 255) / 256 * 256);
    BigBatch b;
    b.Y = Y, b.n = n, b.nch = p.nch, b.sstride = p.sstride, b.NB = p.NB, b.NBT = p.NBT;
    b.ab.B = (u32 *)(w + p.off_ab);                         // per batch: rpb * n words of B, then as many of A
    b.ab.A = b.ab.B + (size_t)p.rpb * n;
    b.ab.H = nullptr;
    b.sorted = (double *)(w + p.off_sorted);
    b.bval = (double *)(w + p.off_bval);
    b.bidx = (u32 *)(w + p.off_bidx);
    b.spl = (double *)(w + p.off_spl);
    b.mk = (double *)(w + p.off_mk);
    b.tab = (u32 *)(w + p.off_tab);
    b.rp = (double2 *)(w + p.off_rp);
    char *zb = b.zero = w + p.off_zero;
    b.zero_bytes = p.zero_bytes;
    b.bcnt = (u32 *)(zb + p.z_bcnt), b.nnanrow = (u32 *)(zb + p.z_nnan), b.ovf = (u32 *)(zb + p.z_ovf);
    b.bflag = (u32 *)(zb + p.z_bflag), b.nanf = (u32 *)(zb + p.z_nanf), b.rowtied = (u32 *)(zb + p.z_tied);
    b.gate = (u32 *)(zb + p.z_gate);
    b.meet = (u32 *)(zb + p.z_meet);
    // A gate word is "set" when it holds the batch's epoch (a process-wide counter, never 0): nothing has to zero it, and
    // stale workspace contents can at worst make the fall-back kernel scan flags that S3 has zeroed -- time, never results.
    static std::atomic<u32> epoch_counter{0};

    // cross-check builds: a retired generation ranks the batches (mbd_rank_big_retired.hip)
    const bool gen2 = xswitch("SD_BIG_GEN2") == 1 || xswitch("SD_BIG_SORT") == 1 || xswitch("SD_BIG_PART1") == 1;
    const bool retired = gen2 || xswitch("SD_BIG_IMPL") == 1;
    // fold mode up to 131 070 curves: the half-word image (cross-check builds, SD_BIG_NOHALF = 1: B words as before; the second
    // generation's packed kernel writes B words only)
    if (!img_out && !gen2 && n <= AB2_H_MAXN && xswitch("SD_BIG_NOHALF") != 1) b.ab.H = (unsigned short *)(w + p.off_h);
    const int NB = p.NB, NBT = p.NBT;
    // The fall-back kernel's workgroups wait for each other: its grid is what the launch's CUs hold at once
    // (one workgroup on each CU the stream may use; a kernel that launches at all fits once), never more.
    const int usable = stream_cus(s);
    unsigned fgrid = (unsigned)(usable < 1 ? 1 : usable);
    if (fgrid > (unsigned)FB_MAXGRID) fgrid = FB_MAXGRID;
    // polls (about a microsecond each) before a waiting workgroup leaves its items to the last arriver; cross-check builds:
    // SD_BIG_SPIN = 1 makes every workgroup but the last give up at once (the take-over path under test)
    u32 spin_limit = 1u << 20;
    if (xswitch("SD_BIG_SPIN") > 0) spin_limit = (u32)xswitch("SD_BIG_SPIN") - 1u;
    // sample per row: 2 048 values up to 24 value buckets (>= 85 samples per bucket), 4 096 up to 72, 16 384 above.
    // The sort of the sample by ONE workgroup is pure latency in front of the partition (4 096 keys: 33 us, as 256 x 16
    // or 1024 x 4 alike), so the sample is no larger than the buckets' capacity margin needs.
    auto k_s3_small = bucket_setup_kernel<128, 16>;
    auto k_s3 = bucket_setup_kernel<256, 16>;
    auto k_s3_big = bucket_setup_kernel<1024, 16>;
    constexpr size_t lds_sp_small = R2Cfg<128, 16>::LDS_BYTES, lds_sp = R2Cfg<256, 16>::LDS_BYTES;
    constexpr size_t lds_sp_big = R2Cfg<1024, 16>::LDS_BYTES;
    const size_t lds_p3 = p3_lds_bytes(NBT);
    SD_HIP(hipFuncSetAttribute((const void *)k_s3_small, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sp_small));
    SD_HIP(hipFuncSetAttribute((const void *)k_s3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sp));
    SD_HIP(hipFuncSetAttribute((const void *)k_s3_big, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sp_big));
    SD_HIP(hipFuncSetAttribute((const void *)bucket_partition3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_p3));
    SD_HIP(hipFuncSetAttribute((const void *)bucket_rank32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)A3_LDS));
    SD_HIP(hipFuncSetAttribute((const void *)big_fallback_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BigCfg::LDS_BYTES));

    for (i64 row0 = 0; row0 < T; row0 += p.rpb) {
        const i64 rows = T - row0 < p.rpb ? T - row0 : p.rpb;
        b.row0 = row0, b.rows = rows;
        const u32 *nn_for_fold = b.nnanrow;
        if (img_out) b.ab.B = img_out + (size_t)row0 * n;    // image mode: the B words straight into the caller's image
        u32 epoch = ++epoch_counter;
        if (epoch == 0) epoch = ++epoch_counter;
        if (retired) {
            const int rc = retired_big_rank_batch(b, s, &nn_for_fold);
            if (rc) return rc;
        } else {
            // ---- S3 -> P3 -> A3 (tied rows: its fp64 form) -> the fall-backs behind their gate words ----
            auto s3 = [&](auto kernel, int threads, size_t lds) {
                hipLaunchKernelGGL(kernel, dim3((unsigned)rows), dim3(threads), lds, s, Y, n, row0, NB, b.spl, b.mk, b.tab, b.rp,
                                   b.rowtied, b.bcnt, b.bflag, b.nnanrow, b.ovf, b.nanf, b.meet);
            };
            if (NB <= S3_SMALL_NB) s3(k_s3_small, 128, lds_sp_small);
            else if (NB <= S3_MID_NB) s3(k_s3, 256, lds_sp);
            else s3(k_s3_big, 1024, lds_sp_big);
            hipLaunchKernelGGL(bucket_partition3_kernel, dim3((unsigned)((n + P3_C - 1) / P3_C), (unsigned)rows), dim3(P3_NT),
                               lds_p3, s, Y, n, row0, NBT, (const double *)b.spl, (const double *)b.mk, (const u32 *)b.tab,
                               (const double2 *)b.rp, (const u32 *)b.rowtied, b.bcnt, b.nnanrow, b.ovf, (u64 *)b.bval, b.bidx,
                               b.gate, epoch, b.ab);
            hipLaunchKernelGGL(bucket_rank32_kernel, dim3((unsigned)(8 * NBT * ((rows + 7) / 8))), dim3(A3_NT), A3_LDS, s, Y, n,
                               row0, rows, NBT, (const u32 *)b.bcnt, (const u32 *)b.nnanrow, (const u32 *)b.ovf,
                               (const u32 *)b.rowtied, (const u64 *)b.bval, (const u32 *)b.bidx, b.bflag, b.gate, epoch, b.ab);
            hipLaunchKernelGGL(big_fallback_kernel, dim3(fgrid), dim3(BIG_NT), BigCfg::LDS_BYTES, s, Y, n, row0, rows, NBT,
                               (const u32 *)b.bcnt, (const u32 *)b.nnanrow, (const u32 *)b.bflag, (const u32 *)b.rowtied,
                               (const double *)b.bval, (const u32 *)b.bidx, b.sorted, p.sstride, b.nanf, (int)p.nch,
                               (const u32 *)b.ovf, (const u32 *)b.gate, epoch, b.meet, spin_limit, b.ab);
            SD_HIP(hipGetLastError());
        }
        if (img_out) {
            SD_HIP(hipMemcpyAsync(nnan_out + row0, nn_for_fold, (size_t)rows * 4, hipMemcpyDeviceToDevice, s));
            continue;
        }
        const int rc = fold_ab2_image(b.ab, nn_for_fold, rows, n, targets, tbegin, m, J, out, row0 == 0, s);
        if (rc) return rc;
    }
    return SD_OK;
}

}  // namespace sd
