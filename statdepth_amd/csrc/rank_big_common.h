// rank_big_common.h -- device code the large-n rank route (mbd_rank_big.hip) shares with its retired generations
// (mbd_rank_big_retired.hip, cross-check library only): the pair image, the chunked route's sort and search, the fp64
// bucket ranking and the sort + search of a flagged bucket, with the constants they need.  Everything here is inlined
// into the kernels of the two files.
#pragma once
#include "sd_common.h"
#include "rank_sort.h"
#include "rank_bucket.h"

namespace sd {

// The pair image of a batch of rows: for every (row, curve) ONE u32 -- B (others strictly below), with bit 31 set when
// the curve ties with another one at this timepoint -- and, for the tied keys only, A (strictly above) in a second
// image; an untied key has A = n_real - 1 - B.  Continuous data writes and reads 4 bytes per key instead of 8 (the
// scattered 8-byte pairs were 596 MB of the ranking kernel's traffic at config 3, profiles/r02_config3_pmc_traffic.json).
struct AB2 {
    u32 *B;
    u32 *A;
    unsigned short *H;                         // half-word image (n <= AB2_H_MAXN, fold mode) or nullptr
};
constexpr u32 AB2_NAN = 0xFFFFFFFFu;           // B word: the curve is NaN at this timepoint
constexpr u32 AB2_TIE = 0x80000000u;           // B word: A is in the second image
// The fold wants C(v, j) - C(A, j) - C(B, j), symmetric in A and B, and an untied key has A + B = nreal - 1: min(A, B) says
// it all and fits 16 bits up to 131 070 curves -- 2 bytes per (row, curve) written and read instead of 4 (config 3: 102 MB
// less traffic).  AB2_H_WORD: look at the B word (NaN, or a tied key with its A in the second image).
constexpr unsigned short AB2_H_WORD = 0xFFFFu;
constexpr i64 AB2_H_MAXN = 131070;

// an untied key: A = nreal - 1 - B
__device__ __forceinline__ void ab_store_untied(const AB2 &ab, size_t idx, u32 B, u32 nreal) {
    if (ab.H) {
        const u32 A = nreal - 1u - B;
        ab.H[idx] = (unsigned short)(A < B ? A : B);
    } else {
        ab.B[idx] = B;
    }
}
__device__ __forceinline__ void ab_store_nan(const AB2 &ab, size_t idx) {
    ab.B[idx] = AB2_NAN;
    if (ab.H) ab.H[idx] = AB2_H_WORD;
}
__device__ __forceinline__ void ab_store(const AB2 &ab, size_t idx, u32 B, u32 A, u32 nreal) {
    if (A + B + 1u == nreal) {
        ab_store_untied(ab, idx, B, nreal);
    } else {
        ab.B[idx] = B | AB2_TIE;
        ab.A[idx] = A;
        if (ab.H) ab.H[idx] = AB2_H_WORD;
    }
}

// =====================================================================================================
// route 2: chunks in curve order
// =====================================================================================================
constexpr int BIG_NT = 1024, BIG_E = 16;
constexpr int BIG_C = BIG_NT * BIG_E;          // 16384 keys per chunk
using BigCfg = R2Cfg<BIG_NT, BIG_E>;

// persistent 1-D grid over (chunk, row); rowflag != nullptr: only rows with a non-zero flag (none: every workgroup reads
// a few flags and leaves)
__device__ __forceinline__ void chunk_sort_items(const double *__restrict__ Y, i64 n, i64 row0, i64 rows, i64 nch,
                                                 double *sorted, i64 sstride, u32 *nanrow,
                                                 const u32 *__restrict__ rowflag, double *Sm) {
    constexpr int E = BIG_E, WB = BigCfg::WB;
    for (i64 v = blockIdx.x; v < rows * nch; v += gridDim.x) {
    const i64 c = v % nch, rb = v / nch;
    if (rowflag && !rowflag[rb]) continue;
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));                               // per-item opaque thread id: no address hoisted out of the loop
    const int lane = t & 63, wave = t >> 6;
    __syncthreads();                                          // the previous item's sort image is no longer in use
    const i64 base = c * BIG_C;
    const int nc = (int)((n - base) < BIG_C ? (n - base) : BIG_C);
    const int n_act = ((nc + WB - 1) / WB) * WB;
    const bool wreal = wave * WB < n_act;
    const double INF = __builtin_huge_val();
    const double *rp = Y + (row0 + rb) * n + base + (wave * WB + lane);
    double k[E];
    u32 mynan = 0;
    if (wreal) {
#pragma unroll
        for (int e = 0; e < E; ++e) k[e] = (wave * WB + lane + e * 64 < nc) ? rp[e * 64] : INF;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            bool isn = k[e] != k[e];
            mynan += isn ? 1u : 0u;
            k[e] = isn ? INF : k[e];
        }
    }
    for (int o = 32; o > 0; o >>= 1) mynan += __shfl_down(mynan, o);
    if (lane == 0 && mynan) atomicAdd(&nanrow[rb], mynan);
    R2Sorter<BIG_NT, BIG_E>::sort(k, Sm, t, n_act, wreal, INF);
    if (wreal) {
        // layout 0: thread t holds sorted positions 16 t .. 16 t + 15 (two 64-byte runs per thread)
        double *dst = sorted + rb * sstride + base + (i64)t * E;
#pragma unroll
        for (int r = 0; r < E; ++r) dst[r] = k[r];
    }
    }
}

// persistent 1-D grid over the items (row, query chunk): the chunk's curves are searched in every sorted chunk of the row
__device__ __forceinline__ void chunk_search_items(const double *__restrict__ Y, i64 n, i64 row0, i64 rows,
                                                   const double *sorted, i64 sstride, const u32 *nanrow, int nchunks,
                                                   const u32 *__restrict__ rowflag, const AB2 &ab, double *Sm,
                                                   i64 vfirst, i64 vstride) {
    constexpr int E = BIG_E, WB = BigCfg::WB, N = BIG_C;
    const double INF = __builtin_huge_val();
    for (i64 v = vfirst; v < rows * nchunks; v += vstride) {
        const i64 rb = v / nchunks;
        if (rowflag && !rowflag[rb]) continue;
        int t = threadIdx.x;
        asm volatile("" : "+v"(t));                           // per-item opaque thread id
        const int qc = (int)(v % nchunks);
        const i64 qbase = (i64)qc * BIG_C;
        const int nq = (int)((n - qbase) < BIG_C ? (n - qbase) : BIG_C);
        const double *xp = Y + (row0 + rb) * n + qbase + t;
        double x[E];
        u32 lo[E], hi[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            x[e] = (t + e * BIG_NT < nq) ? xp[e * BIG_NT] : INF;
            lo[e] = 0;
            hi[e] = 0;
        }
        for (int c = 0; c < nchunks; ++c) {
            const i64 base = (i64)c * BIG_C;
            const int nc = (int)((n - base) < BIG_C ? (n - base) : BIG_C);
            const int n_act = ((nc + WB - 1) / WB) * WB;
            const double *src = sorted + rb * sstride + base;
            __syncthreads();                          // previous chunk's searches are done
            for (int p = t; p < n_act; p += BIG_NT) Sm[r2_swz(p)] = src[p];
            __syncthreads();
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if ((e & 3) == 0) __builtin_amdgcn_sched_barrier(0);
                if (t + e * BIG_NT < nq && x[e] == x[e]) {
                    int l = r2_bound<N, SlotSwz, false>(Sm, n_act, x[e], INF);
                    int h = l;
                    // keys equal to x in this chunk?  (always true once: in x's own chunk)
                    double nx = (l < n_act) ? Sm[r2_swz(l)] : INF;
                    if (l < n_act && nx <= x[e]) h = r2_bound<N, SlotSwz, true>(Sm, n_act, x[e], INF);
                    lo[e] += (u32)l;
                    hi[e] += (u32)h;
                }
            }
        }
        const u32 nnan = nanrow[rb];
        const size_t dst = (size_t)(rb * n + qbase + t);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (t + e * BIG_NT < nq) {
                if (x[e] == x[e])
                    ab_store(ab, dst + e * BIG_NT, lo[e], (x[e] == INF) ? 0u : (u32)(n - hi[e]) - nnan, (u32)n - nnan);
                else
                    ab_store_nan(ab, (size_t)(dst + e * BIG_NT));
            }
        }
    }
}

// =====================================================================================================
// route 1: value buckets
// =====================================================================================================
constexpr int BK_CE = 16;                      // keys per thread of the ranking kernels = bucket capacity / 512
constexpr int BK_NT = 512, BK_E = 16;          // the search kernel's sort: 8 192 slots
constexpr int BK_C = BK_NT * BK_CE;            // bucket capacity (8 192)
static_assert(BK_C <= BK_NT * BK_E, "a value bucket fits the search kernel's sort");
constexpr int BK_MAXNB = 1024;
using BkCfg = R2Cfg<BK_NT, BK_E>;

// A': ranks inside one value bucket WITHOUT a sort, the method of mbd_rank_bucket.hip:
// a monotone map of the bucket's keys onto NBF fine buckets (LDS histogram, the atomic's return value is the slot),
// exclusive prefix sum, scatter into fine-bucket order, and every key counts the members of its own fine bucket that
// are < / <= itself: B = (keys in earlier value buckets) + base + less, A = n_real - (... + base + le).  Ties are exact.
// A value bucket whose keys are all equal is closed-form; one with a fine bucket above BR_CAP keys (heavy ties that
// are not all equal, an infinity stretching the range) is flagged for bucket_search_items.
// w: the item, 8 * NB * ceil(rows / 8) of them (see the mapping below).
constexpr int BR_NT = 512, BR_E = BK_CE, BR_LNB = 12, BR_NBF = 1 << BR_LNB, BR_CAP = 63, BR_TRYB = 4, BR_U2 = 3, BR_PAD = 8;
static_assert(((BR_CAP + 1) & BR_CAP) == 0, "the crowding test reads the counters' bits");
constexpr int BR_NW = BR_NT / 64;
static_assert(BR_NT * BR_E == BK_C, "one thread slot per key of a full value bucket");
static_assert(BR_NBF / 2 / BR_NT == 4, "one 16-byte quad of histogram words per thread");
constexpr size_t BR_HDR = 256;                                         // min/max partials [NW][2] doubles, wave totals [NW]
constexpr size_t BR_LDS = BR_HDR + (size_t)(BR_NBF / 2 + 4) * 4 + (size_t)(BK_C + BR_PAD + 2 * BR_U2 + 4) * 8;

__device__ __forceinline__ void bucket_rank_item(const int w, i64 n, i64 rows, int NB, const u32 *__restrict__ bcnt,
                                                 const u32 *__restrict__ nnanrow, const u32 *__restrict__ ovf,
                                                 const u32 *__restrict__ rowtied, const double *__restrict__ bval,
                                                 const u32 *__restrict__ bidx, u32 *__restrict__ bflag,
                                                 u32 *__restrict__ gate, u32 epoch, AB2 ab) {
    constexpr int E = BR_E, NT = BR_NT, NBF = BR_NBF, NW = BR_NW, U2 = BR_U2;
    extern __shared__ double Sm[];
    double *red = Sm;                                                 // [NW][2]
    u32 *wtot = reinterpret_cast<u32 *>(red + 2 * NW);                // [NW], then the sum of the earlier buckets' counts
    u32 *H = reinterpret_cast<u32 *>(Sm + BR_HDR / 8);                // NBF packed u16 counters, then bases
    double *S = reinterpret_cast<double *>(H + NBF / 2 + 4);          // keys in fine-bucket order + NaN sentinels
    const unsigned short *H16 = reinterpret_cast<const unsigned short *>(H);
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    // XCD-aware mapping (workgroups go to the 8 XCDs round-robin): all value buckets of a row run on ONE XCD, close in
    // time, so the 8-byte pair writes they scatter over that row of the image meet in that XCD's L2 and leave it as
    // whole lines.  grid.x = 8 * NB * ceil(rows / 8).
    const int b = (w >> 3) % NB;
    const i64 rb = (i64)((w >> 3) / NB) * 8 + (w & 7);
    if (rb >= rows) return;
    if (ovf[rb]) return;
    if (rowtied && !rowtied[rb]) return;                              // third generation: only the rows flagged "tied"
    const u32 *rowcnt = bcnt + rb * NB;
    const int cnt = (int)rowcnt[b];
    if (cnt == 0) return;
    const double INF = __builtin_huge_val();
    const double QNAN = __builtin_nan("");
    const size_t slot0 = ((size_t)rb * NB + b) * BK_C;

    // keys of thread t: slots t, t + NT, ... (coalesced); slots beyond cnt read as NaN = "no key"
    double k[E];
    {
        const double *rp = bval + slot0 + t;
#pragma unroll
        for (int e = 0; e < E; ++e) k[e] = (t + e * NT < cnt) ? rp[e * NT] : QNAN;
    }
    // keys in earlier value buckets of this row
    u32 gsum = 0;
    for (int q = t; q < b; q += NT) gsum += rowcnt[q];
    gsum = rb_wave_incl_scan(gsum);
    // LDS setup: empty histogram, sentinels behind the last key
    reinterpret_cast<uint4 *>(H)[t] = make_uint4(0, 0, 0, 0);
    if (t < 4) H[NBF / 2 + t] = 0;
    if (t < BR_PAD + 2 * U2 + 4) S[cnt + t] = QNAN;
    // range
    double mn = INF, mx = -INF;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (e * NT >= cnt) break;                                     // block-uniform: key slots beyond the bucket's fill
        mn = rb_mm<false>(mn, k[e]);
        mx = rb_mm<true>(mx, k[e]);
    }
    mn = rb_wave_allreduce<false>(mn);
    mx = rb_wave_allreduce<true>(mx);
    if (lane == 63) { red[2 * wave] = mn; red[2 * wave + 1] = mx; wtot[wave] = gsum; }
    __syncthreads();                                                  // barrier 1
    double lo, hi;
    u32 gbase;
    {
        const double2 p = reinterpret_cast<const double2 *>(red)[lane & (NW - 1)];
        lo = rb_readlane_f64(rb_row_allreduce<false>(p.x), 0);        // rotations over 16 lanes see each of the 8 twice
        hi = rb_readlane_f64(rb_row_allreduce<true>(p.y), 0);
        const u32 g = (lane < NW) ? wtot[lane] : 0u;
        gbase = rb_readlane(rb_row_incl_scan(g), 15);
    }
    const u32 nreal = (u32)n - nnanrow[rb];
    const size_t abrow = (size_t)(rb * n);
    const u32 *idp = bidx + slot0 + t;
    if (!(hi > lo)) {
        // every key of the bucket has the same value (or there is one key): all tied
        if (hi == lo) {
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (t + e * NT < cnt) ab_store(ab, abrow + idp[e * NT], gbase, nreal - gbase - (u32)cnt, nreal);
        } else if (t == 0) { bflag[rb * NB + b] = 1u; if (gate) gate[0] = epoch; }                   // a signalling NaN poisoned the range: sort it
        return;
    }
    const double scale = (double)NBF / (hi - lo);                     // infinite range -> 0 -> one crowded fine bucket
    if (!(scale < INF)) {                                             // block-uniform: denormal range
        if (t == 0) { bflag[rb * NB + b] = 1u; if (gate) gate[0] = epoch; }
        return;
    }
    // ---- (1) fine bucket + slot ----
    u32 bs[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (e * NT >= cnt) break;
        const double x = k[e];
        double u = (x - lo) * scale;
        u = u > 0.0 ? u : 0.0;                                        // -inf (and NaN) -> 0
        u = u < (double)(NBF - 1) ? u : (double)(NBF - 1);
        u32 fb = (u32)u;
        fb = (x == x) ? fb : (u32)(NBF + 2);                          // no key: dummy counter
        const u32 sh = (fb & 1u) * 16u;
        const u32 old = atomicAdd(&H[fb >> 1], 1u << sh);
        bs[e] = fb | (((old >> sh) & 0xFFFFu) << 16);
    }
    __syncthreads();                                                  // barrier 2
    // ---- (2) exclusive prefix sum; a fine bucket of 2^BR_TRYB keys or more: ties?  (checked behind the scatter) ----
    bool anyover = false, anytry = false;
    {
        const uint4 hq = reinterpret_cast<const uint4 *>(H)[t];
        // some counter > BR_CAP / >= 2^BR_TRYB: bit k of a half-word of the OR is set iff some counter has it
        constexpr u32 HIM = (0xFFFFu & ~(u32)BR_CAP) * 0x10001u, TRM = (0xFFFFu & ~((1u << BR_TRYB) - 1u)) * 0x10001u;
        const u32 s4 = hq.x + hq.y + hq.z + hq.w;
        const u32 ov = hq.x | hq.y | hq.z | hq.w;
        const u32 run = (s4 & 0xFFFFu) + (s4 >> 16);
        const u32 incl = rb_wave_incl_scan(run);
        const bool wover = __ballot((ov & HIM) != 0) != 0, wtry = __ballot((ov & TRM) != 0) != 0;
        if (lane == 63) wtot[wave] = incl | (wover ? 0x80000000u : 0u) | (wtry ? 0x40000000u : 0u);
        __syncthreads();                                              // barrier 3
        const u32 wt = (lane < NW) ? wtot[lane] : 0u;
        anyover = __ballot((wt >> 31) != 0) != 0;                     // block-uniform
        anytry = __ballot((wt & 0x40000000u) != 0) != 0;
        const u32 wscan = rb_row_incl_scan(wt & 0x3FFFFFFFu);
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
    __syncthreads();                                                  // barrier 4
    // ---- (3) scatter into fine-bucket order ----
    u32 bc[E];                                                        // base | count << 16; count 0: no key
    const u32 dummy = (u32)(cnt + BR_PAD + 1) & ~1u;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (e * NT >= cnt) break;
        const u32 fb = bs[e] & 0xFFFFu, slot = bs[e] >> 16;
        const u32 base = H16[fb], end = H16[fb + 1];
        const bool isk = fb < (u32)NBF;
        S[isk ? base + slot : dummy] = k[e];
        bc[e] = isk ? (base | ((end - base) << 16)) : 0u;
    }
    __syncthreads();                                                  // barrier 5
    if (anytry) {                                                     // block-uniform
        // tie-heavy data: when every fine bucket holds ONE value, less = 0 and le = count -- no member pass.
        // Else: the normal way, or the search kernel when a fine bucket is above BR_CAP keys.
        bool pure = true;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (e * NT >= cnt) break;
            if (bc[e] >> 16) pure = pure && (S[bc[e] & 0xFFFFu] == k[e]);
        }
        if (__syncthreads_and(pure)) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (e * NT >= cnt) break;
                const u32 base = bc[e] & 0xFFFFu, fc = bc[e] >> 16;
                if (fc) ab_store(ab, abrow + idp[e * NT], gbase + base, nreal - (gbase + base + fc), nreal);
            }
            return;
        }
        if (anyover) {
            if (t == 0) { bflag[rb * NB + b] = 1u; if (gate) gate[0] = epoch; }
            return;
        }
    }
    // ---- (4) rank inside the fine bucket (the keys are still in registers), write the pairs ----
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (e * NT >= cnt) break;
        if ((e & 1) == 0) __builtin_amdgcn_sched_barrier(0);
        const u32 base = bc[e] & 0xFFFFu, fc = bc[e] >> 16;
        const u32 odd = base & 1u;
        const double x = k[e];
        const double2 *Sq = reinterpret_cast<const double2 *>(S + (base - odd));
        u32 less = 0, le = 0;
#pragma unroll
        for (int u = 0; u < U2; ++u) {
            const double2 y = Sq[u];
            less += (y.x < x) ? 1u : 0u;
            le += (y.x <= x) ? 1u : 0u;
            less += (y.y < x) ? 1u : 0u;
            le += (y.y <= x) ? 1u : 0u;
        }
        less -= odd;
        le -= odd;
        if (fc + odd > (u32)(2 * U2)) {                               // a fine bucket longer than the window
            for (u32 kk = 2 * U2; kk < fc + odd; kk += 2) {
                const double2 y = Sq[kk >> 1];
                less += (y.x < x) ? 1u : 0u;
                le += (y.x <= x) ? 1u : 0u;
                less += (y.y < x) ? 1u : 0u;
                le += (y.y <= x) ? 1u : 0u;
            }
        }
        if (fc) ab_store(ab, abrow + idp[e * NT], gbase + base + less, nreal - (gbase + base + le), nreal);
    }
}

// B: persistent 1-D grid over the (row, bucket) pairs, flagged buckets only (nothing flagged: every workgroup reads a few
// flags and leaves).  rowtied == nullptr or rowtied[row]: fp64 records (bval, bidx); else 8-byte records whose keys are
// gathered from the matrix through their curve indices.
template <int NT, int E>
__device__ __forceinline__ void bucket_search_items(const double *__restrict__ Y, i64 n, i64 row0, i64 rows, int NB,
                                                    const u32 *__restrict__ bcnt, const u32 *__restrict__ nnanrow,
                                                    const u32 *__restrict__ bflag, const u32 *__restrict__ rowtied,
                                                    const double *__restrict__ bval, const u32 *__restrict__ bidx,
                                                    const AB2 &ab, double *Sm) {
    using C = R2Cfg<NT, E>;
    constexpr int LE = C::LE, WB = C::WB, N = C::N;
    static_assert(NT * E >= BK_C, "a value bucket fits the sort");
    __shared__ u32 s_basecnt;
    const u64 *rec = reinterpret_cast<const u64 *>(bval);
    for (i64 v = blockIdx.x; v < rows * NB; v += gridDim.x) {
        if (!bflag[v]) continue;                                      // block-uniform
        int t = threadIdx.x;
        asm volatile("" : "+v"(t));                                   // per-item opaque thread id
        const int lane = t & 63, wave = t >> 6;
        const int b = (int)(v % NB);
        const i64 rb = v / NB;
        const bool packed = rowtied && !rowtied[rb];
        const double *yrow = Y + (row0 + rb) * n;
        const int cnt = (int)bcnt[rb * NB + b];
        __syncthreads();                                              // the previous item's image is no longer read
        if (t == 0) {
            u32 sum = 0;
            for (int q = 0; q < b; ++q) sum += bcnt[rb * NB + q];
            s_basecnt = sum;
        }
        const int n_act = ((cnt + WB - 1) / WB) * WB;
        const bool wreal = wave * WB < n_act;
        const double INF = __builtin_huge_val();
        const size_t slot0 = ((size_t)rb * NB + b) * BK_C;
        const int i0 = wave * WB + lane;
        double k[E];
        if (wreal) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int j = i0 + e * 64;
                k[e] = (j < cnt) ? (packed ? yrow[(u32)(rec[slot0 + j] >> 32)] : bval[slot0 + j]) : INF;
            }
        }
        R2Sorter<NT, E>::sort(k, Sm, t, n_act, wreal, INF);
        if (wreal) {
            double *Sw = Sm + r2_base<0, LE>(t);
#pragma unroll
            for (int e = 0; e < E; ++e) Sw[r2_off<0, LE>(e)] = k[e];
        }
        __syncthreads();
        const u32 base = s_basecnt;
        const u32 nreal = (u32)n - nnanrow[rb];
        for (int j = t; j < cnt; j += NT) {
            const u32 id = packed ? (u32)(rec[slot0 + j] >> 32) : bidx[slot0 + j];
            const double x = packed ? yrow[id] : bval[slot0 + j];
            int lo = r2_bound<N, SlotPad<LE>, false, false>(Sm, n_act, x, INF);       // x is in the bucket
            int hi = lo + 1, step = 1;
            while (hi + step <= n_act && Sm[r2_phys<LE>(hi + step - 1)] <= x) { hi += step; step <<= 1; }
            while (step > 1) {
                step >>= 1;
                if (hi + step <= n_act && Sm[r2_phys<LE>(hi + step - 1)] <= x) hi += step;
            }
            // values above x: everything real beyond x's tie run (x = +inf: the padding ties with it, nothing is above)
            ab_store(ab, (size_t)(rb * n + id), base + (u32)lo, (x == INF) ? 0u : nreal - (base + (u32)hi), nreal);
        }
    }
}

// One batch of rows of the large-n route and the blocks big_run carved from the workspace for it (BigPlan,
// mbd_rank_big.hip); what the hook of the retired generations gets (rank_routes.h).
struct BigBatch {
    const double *Y;
    i64 n, row0, rows, nch, sstride;
    int NB, NBT;                                         // interior value buckets; NBT = NB + 2 with the two end buckets
    AB2 ab;
    double *sorted, *bval, *spl, *mk;
    u32 *bidx, *tab;
    double2 *rp;
    char *zero;                                          // the zeroed block (S3 zeroes it; the retired generations memset): the words below
    size_t zero_bytes;
    u32 *bcnt, *nnanrow, *ovf, *bflag, *nanf, *rowtied, *gate, *meet;
};

}  // namespace sd
