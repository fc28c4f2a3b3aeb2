// mbd_rank_bucket.hip -- K1+K2 rank formulation without a sort (default path of sd_mbd_counts, 2 <= n <= 16384, J <= 3).
//
// Same integers as the pairwise kernel and the reference's enumeration (_functional.py:246-251,
// _containment.py:75-77): per (curve, timepoint) the counts B (others strictly below) and A (strictly above),
// folded as C(n-1,j) - C(A,j) - C(B,j) over t.  A rank needs no sorted row, only "how many keys are below
// mine", and that splits into a coarse part any monotone bucketing answers with a histogram and a fine part
// that only the few keys sharing my bucket can change:
//
//   F  rank_bucket_kernel   -- one workgroup per row (persistent over rows g, g+G, ...), thread t owns curves
//      t, t+NT, ... for the whole launch.  Per row: (0) min/max of the row; (1) bucket b(x) = floor((x-lo) *
//      NB/(hi-lo)) -- rounding is monotone, so b is a non-decreasing function of x whatever the data -- and one
//      LDS atomic per key on a packed u16 histogram, whose return value is the key's slot inside its bucket;
//      (2) exclusive prefix sum of the NB counters; (3) keys scattered into bucket order; (4) every key
//      compares itself with the members of its own bucket: B = base + #(y < x), A = n - base - #(y <= x).
//      Keys past the end of a bucket belong to later buckets and compare greater (NaN sentinels follow the
//      last one), so the member loop needs no bounds.  Ties are exact by construction (equal values share a bucket).  The per-curve band counts
//      are accumulated in REGISTERS across the workgroup's rows; one partial total per (workgroup, curve)
//      goes to HBM at the end: the matrix is read once and nothing per (row, curve) is ever written.
//      NaNs stay out of the histogram and weigh in as pandas' skipna does; +-inf take the end buckets.
//      Tie-heavy rows (a bucket of 16 keys or more): when every bucket of the row holds ONE value -- quantised or
//      integer data, a row of equal values -- the ranks are closed form (less = 0, le = count) and the row needs no
//      member pass at all.  A row with an infinity, or with a bucket above CAP keys that mixes values, is set aside
//      and sorted by the same workgroup behind its row loop (rb_slow_row).
//      Rows much wider than their bulk (heavy tails, outlying curves): a row whose histogram shows a crowded bucket and
//      whose range exceeds the central bracket of its threads' own keys many times over is histogrammed again under the
//      three-piece map of rank_bucket.h (linear core + float-like tails, monotone for any data); the rows behind it take
//      their bracket with their range.  The external-target and medium kernels (mbd_rank_external.hip, mbd_rank_medium.hip)
//      use the same map, through the row build of rank_bucket_row.h; the LDS layout of a row (RBCfg) is there too.
//   Z  rank_finalize_kernel / rank_finalize4_kernel -- totals of the requested targets = sum of the workgroups'
//      partials (+ the fold of pair-image rows when the caller supplies one).
//
// HBM traffic per call: the matrix once (8 nT) + G partials of 8 n (J-1) bytes written and read once.
#include <type_traits>

#include "sd_common.h"
#include "rank_routes.h"
#include "rank_sort.h"
#include "rank_bucket_row.h"
#include "rank_fold.h"

namespace sd {

// ---------------------------------------------------------------------------------------------------
// The row the bucket map cannot spread (an infinite bracket, a crowded bucket that mixes values): in-LDS sort of the
// plain values + binary search, the method of rank_search_kernel (mbd_rank_ab.hip), for ONE row inside the
// bucket kernel, run behind the main row loop for the rows it set aside.  Thread t gets the pairs
// of its curves t + 1024 e in ab[e] (B | A << 16, AB_SPECIAL where the curve is NaN or beyond n).
// The sort image overlays the LDS at Sm; s_cnt is one LDS word outside it.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rb_slow_row(const double *__restrict__ row, int n, double *Sm, u32 *s_cnt, u32 *ab,
                                         u32 *nnan_out) {
    using SC = R2Cfg<RB_SNT, RB_SE>;
    using Sorter = R2Sorter<RB_SNT, RB_SE>;
    constexpr int N = SC::N, LE = SC::LE, WB = SC::WB;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n_act = ((n + WB - 1) / WB) * WB;
    const bool wreal = wave * WB < n_act;
    const double INF = __builtin_huge_val();
    if (t == 0) *s_cnt = 0;
    __syncthreads();
    double k[RB_SE];
    u32 mynan = 0;
    if (wreal) {
        const int i0 = wave * WB + lane;
#pragma unroll
        for (int e = 0; e < RB_SE; ++e) {
            double x = (i0 + e * 64 < n) ? row[i0 + e * 64] : INF;
            const bool isn = x != x;                                  // NaN -> +inf, counted (pandas skipna)
            mynan += isn ? 1u : 0u;
            k[e] = isn ? INF : x;
        }
    }
    if (mynan) atomicAdd(s_cnt, mynan);
    Sorter::sort(k, Sm, t, n_act, wreal, INF);
    if (wreal) {
        double *Sw = Sm + r2_base<0, LE>(t);
#pragma unroll
        for (int e = 0; e < RB_SE; ++e) Sw[r2_off<0, LE>(e)] = k[e];
    }
    __syncthreads();
    const u32 nnan = *s_cnt;
#pragma unroll 4
    for (int e = 0; e < RB_SE; ++e) {
        u32 r = AB_SPECIAL;
        if (t + e * RB_SNT < n) {
            const double x = row[t + e * RB_SNT];
            if (x == x) {
                const int lo = r2_bound<N, SlotPad<LE>, false, false>(Sm, n_act, x, INF);   // x is in the row
                int hi = lo + 1, step = 1;                            // gallop over the tie run of x
                while (hi + step <= n_act && Sm[r2_phys<LE>(hi + step - 1)] <= x) { hi += step; step <<= 1; }
                while (step > 1) {
                    step >>= 1;
                    if (hi + step <= n_act && Sm[r2_phys<LE>(hi + step - 1)] <= x) hi += step;
                }
                // keys <= x within [0, n_act) are real non-NaN values unless x = +inf
                const u32 A = (x == INF) ? 0u : (u32)(n - hi) - nnan;
                r = (u32)lo | (A << 16);
            }
        }
        ab[e] = r;
    }
    *nnan_out = nnan;
    __syncthreads();                                                  // the image is free again
}

// SEL (J == 2, every curve a target): the second and last launch behind rank_bucket32_kernel (mbd_rank_bucket32.hip).
// (1) Each workgroup sums its slice of curves over that kernel's Gsum u32 partial blocks and adds the totals to out_tot
// (zeroed by rank_bucket32_kernel) -- the finalize step, without a launch of its own.  (2) Only when that kernel flagged
// rows (*gate == epoch; else return): the flagged rows are ranked here in fp64 and their band counts added to out_tot
// as well.  Every workgroup derives the same ordered list of flagged rows and takes entries g, g + G, ...
template <int NT, int E, int LNB, int J, int CAP, int U2, bool A32 = false, bool SEL = false>
__global__ __launch_bounds__(NT, 4) void rank_bucket_kernel(const double *__restrict__ Y, i64 n64, i64 row0, i64 rows,
                                                         u64 *__restrict__ partial, int p32, u32 *__restrict__ nnan_img,
                                                         const unsigned char *__restrict__ rowflag = nullptr,
                                                         const u32 *__restrict__ gate = nullptr, u32 epoch = 0,
                                                         u64 *__restrict__ out_tot = nullptr, int Gsum = 0,
                                                         u32 *__restrict__ fblocks = nullptr, u32 *__restrict__ done = nullptr,
                                                         int kspin = 1) {
    // J == 0: image mode (J >= 4 on the host side): no fold, the pairs (B | A << 16) of every (row, curve) go to the
    // pair image `partial` (as u32[rows][n]) and the rows' NaN counts to nnan_img; rank_accumulate*_kernel folds them
    using C = RBCfg<NT, E, LNB, U2>;
    constexpr int NB = C::NB, NW = C::NW, QW = C::QW;
    static_assert(2 * U2 - 1 <= RB_PAD, "the first member pass reads at most RB_PAD keys past the end");
    static_assert(CAP == 127 && NB <= 32768, "packing of (base, count, slot); the crowding test reads the counters' bits");
    constexpr int TRYB = (E == 16) ? 5 : 4;     // buckets of 16 (32 at NB = 8192 / n > 15360) keys: ties rather than density
    constexpr int NACC = (J == 2 || J == 0) ? 1 : (J - 1);
    u32 *ABimg = reinterpret_cast<u32 *>(partial);
    extern __shared__ double Sm[];
    const int n = (int)n64;
    double *red = Sm;                                                 // [2][NW][2] min/max partials
    u32 *wtot = reinterpret_cast<u32 *>(red + 4 * NW);                // [NW]
    u32 *defer = wtot + NW;                                           // [DEFW] bitmap of the rows set aside
    float2 *brk = reinterpret_cast<float2 *>(wtot + C::BRK_WORD);     // [3][NW] the waves' brackets: two parities + the second try
    // histogram before the keys: every LDS offset except the keys' end is a compile-time constant
    u32 *H = reinterpret_cast<u32 *>(Sm + C::HDR / 8);                // NB packed u16 counters, then bases
    double *S = reinterpret_cast<double *>(H + NB / 2 + 4);           // keys in bucket order + sentinels + dummy
    double *IMG = reinterpret_cast<double *>(H);                      // sort image of the rows set aside (overlays both)
    const unsigned short *H16 = reinterpret_cast<const unsigned short *>(H);
    const int t0 = threadIdx.x;
    const double INF = __builtin_huge_val();
    const double QNAN = __builtin_nan("");
    const int DUMMY = C::dummy_pos(n);
    const double2 *NANP = reinterpret_cast<const double2 *>(S + ((n + 1) & ~1));   // two of the sentinels, 16-byte aligned
    int t = t0;
    // SEL: the ordered list of flagged rows behind everything else in LDS (u16 row indices, rows <= 4096)
    const unsigned short *sel = reinterpret_cast<const unsigned short *>(reinterpret_cast<const char *>(Sm) + C::lds_bytes(n));
    if constexpr (SEL) {
        static_assert(!SEL || (J == 2 && A32 && NT == RB_SNT), "second launch behind the 32-bit kernel: J = 2, u32 totals");
        {   // (1) finalize: totals of this workgroup's slice of curves = sum of the Gsum partial blocks (16-byte loads)
            const u32 *P = reinterpret_cast<const u32 *>(partial);
            u64 *redl = reinterpret_cast<u64 *>(Sm);                  // [64 slices][16 quads][4]
            // the blocks lie nst words apart, on 128-byte lines whatever n; a workgroup's slice is whole lines (8 quads), so that no
            // line is fetched by two workgroups (a slice of 10 quads straddled three lines, shared with the neighbours)
            const int nst = (n + 31) & ~31, nq = (n + 3) >> 2, nl = (nq + 7) >> 3;
            const int l0 = (int)((i64)blockIdx.x * nl / gridDim.x), l1 = (int)((i64)(blockIdx.x + 1) * nl / gridDim.x);
            const int q0 = 8 * l0 < nq ? 8 * l0 : nq, q1 = 8 * l1 < nq ? 8 * l1 : nq;
            const int qx = t0 & 15, y = t0 >> 4;
            for (int qb = q0; qb < q1; qb += 16) {
                u64 a0 = 0, a1 = 0, a2 = 0, a3 = 0;
                if (qb + qx < q1) {
                    const u32 *pp = P + 4 * (qb + qx);
#pragma unroll 4
                    for (int g = y; g < Gsum; g += 64) {
                        const uint4 v = *reinterpret_cast<const uint4 *>(pp + (size_t)g * nst);
                        a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
                    }
                }
                u64 *rl = redl + ((size_t)y * 16 + qx) * 4;
                rl[0] = a0; rl[1] = a1; rl[2] = a2; rl[3] = a3;
                __syncthreads();
                if (t0 < 64 && qb + (t0 >> 2) < q1 && 4 * (qb + (t0 >> 2)) + (t0 & 3) < n) {
                    u64 tot = 0;
#pragma unroll 8
                    for (int k = 0; k < 64; ++k) tot += redl[((size_t)k * 16 + (t0 >> 2)) * 4 + (t0 & 3)];
                    atomicAdd(&out_tot[4 * (qb + (t0 >> 2)) + (t0 & 3)], tot);
                }
                __syncthreads();
            }
        }
        if (*gate != epoch) return;                                   // (2) nothing was flagged
        unsigned short *selw = const_cast<unsigned short *>(sel);
        u32 nsel = 0;
        for (i64 c0 = 0; c0 < rows; c0 += NT) {
            const bool f = (c0 + t0 < rows) && rowflag[c0 + t0];
            const u64 m = __ballot(f);
            if ((t0 & 63) == 0) wtot[t0 >> 6] = (u32)__popcll(m);
            __syncthreads();
            u32 off = nsel, tot = 0;
            for (int w = 0; w < NW; ++w) {
                const u32 c = wtot[w];
                off += (w < (t0 >> 6)) ? c : 0u;
                tot += c;
            }
            if (f) selw[off + (u32)__popcll(m & ((1ull << (t0 & 63)) - 1ull))] = (unsigned short)(c0 + t0);
            nsel += tot;
            __syncthreads();
        }
        rows = nsel;                                                  // from here on "row r" is the r-th flagged row
    }
    auto rowptr = [&](i64 r) -> const double * {
        if constexpr (SEL) return Y + (row0 + (i64)sel[r]) * n;
        else return Y + (row0 + r) * n;
    };

    // LDS setup (once, and again behind rb_slow_row): sentinels + dummy range, empty histogram
    auto lds_setup = [&]() {
        for (int p = n + t; p < (int)C::keys_slots(n); p += NT) S[p] = QNAN;
        uint4 *Hq = reinterpret_cast<uint4 *>(H);
#pragma unroll
        for (int i = 0; i < QW; ++i) Hq[i * NT + t] = make_uint4(0, 0, 0, 0);
        if (t < 4) H[NB / 2 + t] = 0;
    };
    lds_setup();
    if (t < C::DEFW) defer[t] = 0;
    u32 ndefer = 0, rowidx = 0;                                       // block-uniform

    // curves of thread t: t, t + NT, ...; slots beyond n read as NaN and are treated like any other NaN
    double k[E];
    auto load_row = [&](i64 r) {
        const double *rp = rowptr(r) + t;
#pragma unroll
        for (int e = 0; e < E; ++e) k[e] = (e < E - 1 || t + (E - 1) * NT < n) ? rp[e * NT] : QNAN;
    };
    // J == 2: acc[e][0] = 2 * (sum of band counts) (one accumulator, see the fold below); else acc[e][j-2].
    // A32 (J == 2, p32 == 2: the host found ceil(rows / G) * n^2 < 2^32): 32-bit accumulators -- E registers fewer
    static_assert(!A32 || J == 2, "32-bit accumulators: J == 2 only");
    using ACC = std::conditional_t<A32, u32, u64>;
    ACC acc[E][NACC];
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int j = 0; j < NACC; ++j) acc[e][j] = 0;

    bool heavy = false;                                               // block-uniform: the last row went under the three-piece map
    // (0) range of a row = min / max of its keys (NaN never wins: pandas skipna, _containment.py:68-69), per wave into
    // LDS.  It is computed for the NEXT row at the end of every iteration, where its VALU work fills the waits of
    // the LDS-bound member passes, and once here for the first row.
    auto row_range = [&](int parity) {
        double mn = INF, mx = -INF;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            mn = rb_mm<false>(mn, k[e]);
            mx = rb_mm<true>(mx, k[e]);
        }
        if (heavy) {                                                  // block-uniform: the bracket of a row that follows a clipped one
            const float2 wb = rb3_wave_bracket<E, NT>(mn, mx);        // (from the threads' own extremes, before they merge)
            if ((t & 63) == 63) brk[parity * NW + (t >> 6)] = wb;
        }
        mn = rb_wave_allreduce<false>(mn);
        mx = rb_wave_allreduce<true>(mx);
        double *rp = red + parity * 2 * NW;
        if ((t & 63) == 63) { rp[2 * (t >> 6)] = mn; rp[2 * (t >> 6) + 1] = mx; }
    };
    int par = 0;
    if ((i64)blockIdx.x < rows) {
        load_row(blockIdx.x);
        row_range(0);
    }
    for (i64 r = blockIdx.x; r < rows; r += gridDim.x) {
        const i64 rnext = r + gridDim.x;
        // Per-row opaque copy of the thread id: every address below derives from it, so the compiler recomputes
        // those few ALU ops per row instead of hoisting loop-invariant address registers out of the row loop
        // and spilling the accumulators to make room (same device as in mbd_rank_ab.hip).
        t = t0;
        asm volatile("" : "+v"(t));
        const int lane = t & 63;
        const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
        double *redp = red + par * 2 * NW;
        const float2 *brkp = brk + par * NW;
        par ^= 1;
        __syncthreads();                                              // barrier 1 (histogram is zero, S is free)
        double lo, hi;
        {
            const double2 p = reinterpret_cast<const double2 *>(redp)[lane & (NW - 1)];
            lo = rb_readlane_f64(rb_row_allreduce<false>(p.x), 0);
            hi = rb_readlane_f64(rb_row_allreduce<true>(p.y), 0);
        }
        // range overflow -> 0 -> one crowded bucket; all values equal -> 0 -> one bucket of one value (closed form below)
        const double scale = (hi > lo) ? (double)NB / (hi - lo) : 0.0;
        // Every decision below is block-uniform.  The next row is loaded at ONE place (two load sites would
        // keep two copies of the key registers alive across the loop).  A row with an infinity or without any
        // value is set aside for the sort behind the loop.
        const bool go = (hi >= lo) && (scale < INF) && (lo > -INF) && (hi < INF);
        u32 bs[E];
        u32 nn = 0;                                                   // NaN others of this row (block-uniform)
        // block-uniform: a bucket above CAP keys / a bucket of 2^TRYB keys or more (ties?  see the member phase)
        bool crowded = false, trypure = false;
        // A row whose range is much wider than its bulk (heavy tails, outlying curves) goes under the three-piece map of
        // rank_bucket.h.  Such a row shows in the histogram of the linear map (a bucket of 2^TRYB keys or more, below) and is
        // histogrammed again; rows of one matrix resemble each other, so after the first one (`heavy`) the bracket is taken
        // with the row's range, BEFORE the histogram, until a row needs no clipping again.  Rows that spread well pay nothing.
        auto bracket_map = [&]() -> Rb3 {
            double mn = INF, mx = -INF;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                mn = rb_mm<false>(mn, k[e]);
                mx = rb_mm<true>(mx, k[e]);
            }
            const float2 wb = rb3_wave_bracket<E, NT>(mn, mx);
            if (lane == 63) brk[2 * NW + wave] = wb;
            __syncthreads();
            return rb3_make<NB>(lo, hi, brk[2 * NW + (lane & (NW - 1))], n);
        };
        auto histogram_clip = [&](const Rb3 &m3) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double x = k[e];
                u32 b = rb3_bucket<NB>(m3, x);
                b = (x == x) ? b : (u32)(NB + 2);
                const u32 sh = (b & 1u) * 16u;
                const u32 old = atomicAdd(&H[b >> 1], 1u << sh);
                bs[e] = b | (((old >> sh) & 0xFFFFu) << 16);
            }
        };
        if (go) {
            Rb3 m3;
            m3.clip = false;
            if (heavy) {                                              // block-uniform: the bracket came with the range
                m3 = rb3_make<NB>(lo, hi, brkp[lane & (NW - 1)], n);
                heavy = m3.clip;
            }
            // ---- (1) bucket + slot, branch-free.  min(fl(fl(x - lo) * scale), NB-1), negative -> 0, is non-decreasing
            //      in x for ANY lo and scale >= 0; NaNs count into a dummy word behind the histogram ----
            if (m3.clip) histogram_clip(m3);
            else
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double x = k[e];
                double u = (x - lo) * scale;
                u = u < (double)(NB - 1) ? u : (double)(NB - 1);      // NaN -> NB-1 (overridden below)
                u32 b;
                asm("v_cvt_u32_f64 %0, %1" : "=v"(b) : "v"(u));       // saturating: below the range -> bucket 0
                b = (x == x) ? b : (u32)(NB + 2);
                const u32 sh = (b & 1u) * 16u;
                const u32 old = atomicAdd(&H[b >> 1], 1u << sh);
                bs[e] = b | (((old >> sh) & 0xFFFFu) << 16);
            }
            __syncthreads();                                          // barrier 2
            uint4 *Hq = reinterpret_cast<uint4 *>(H) + wave * (64 * QW);   // this wave's 64*QW quads, quad i*64+lane
            {
                // ---- (2) exclusive prefix sum over the counters (conflict-free 16-byte accesses: lane <-> quad);
                //      a crowded bucket defers the row ----
                uint4 hq[QW];
                u32 runq[QW], inclq[QW], offq[QW];
                auto prefix_a = [&]() {
                    u32 ov = 0, wsum = 0;
#pragma unroll
                    for (int i = 0; i < QW; ++i) {
                        hq[i] = Hq[i * 64 + lane];
                        const u32 s4 = hq[i].x + hq[i].y + hq[i].z + hq[i].w;   // both halves at once: no half exceeds 16384
                        ov |= hq[i].x | hq[i].y | hq[i].z | hq[i].w;            // bit k of a half set <=> some counter has it
                        runq[i] = (s4 & 0xFFFFu) + (s4 >> 16);
                        inclq[i] = rb_wave_incl_scan(runq[i]);
                        offq[i] = wsum;
                        wsum += rb_readlane(inclq[i], 63);
                    }
                    // some counter > CAP (= 2^7 - 1) / some counter >= 2^TRYB: any of the bits from there up is set
                    constexpr u32 HIM = (0xFFFFu & ~(u32)CAP) * 0x10001u, TRM = (0xFFFFu & ~((1u << TRYB) - 1u)) * 0x10001u;
                    const bool wover = __ballot((ov & HIM) != 0) != 0, wtry = __ballot((ov & TRM) != 0) != 0;
                    if (lane == 63) wtot[wave] = wsum | (wover ? 0x80000000u : 0u) | (wtry ? 0x40000000u : 0u);
                };
                prefix_a();
                __syncthreads();                                      // barrier 3
                u32 wt = wtot[lane & (NW - 1)];
                crowded = __ballot((wt >> 31) != 0) != 0;
                trypure = __ballot((wt & 0x40000000u) != 0) != 0;
                if (__ballot((wt & 0x40000000u) != 0) != 0 && !m3.clip) {   // block-uniform, rare
                    // A bucket of 2^TRYB keys or more under the linear map: tie-heavy data -- or a range much wider than the
                    // row's bulk.  The bracket tells them apart; the second kind is histogrammed again under core + tails.
                    m3 = bracket_map();
                    if (m3.clip) {                                    // block-uniform
                        heavy = true;
#pragma unroll
                        for (int i = 0; i < QW; ++i) Hq[i * 64 + lane] = make_uint4(0, 0, 0, 0);
                        if (t < 4) H[NB / 2 + t] = 0;
                        __syncthreads();
                        histogram_clip(m3);
                        __syncthreads();
                        prefix_a();
                        __syncthreads();
                        wt = wtot[lane & (NW - 1)];
                        crowded = __ballot((wt >> 31) != 0) != 0;
                        trypure = __ballot((wt & 0x40000000u) != 0) != 0;
                    }
                }
                const u32 wscan = rb_row_incl_scan(wt & 0x3FFFFFFFu);
                const u32 woff = wave ? rb_readlane(wscan, wave - 1) : 0u;
#pragma unroll
                for (int i = 0; i < QW; ++i) {
                    u32 base = woff + offq[i] + inclq[i] - runq[i];
                    uint4 o;
                    o.x = base | ((base + (hq[i].x & 0xFFFFu)) << 16);
                    base += (hq[i].x & 0xFFFFu) + (hq[i].x >> 16);
                    o.y = base | ((base + (hq[i].y & 0xFFFFu)) << 16);
                    base += (hq[i].y & 0xFFFFu) + (hq[i].y >> 16);
                    o.z = base | ((base + (hq[i].z & 0xFFFFu)) << 16);
                    base += (hq[i].z & 0xFFFFu) + (hq[i].z >> 16);
                    o.w = base | ((base + (hq[i].w & 0xFFFFu)) << 16);
                    base += (hq[i].w & 0xFFFFu) + (hq[i].w >> 16);
                    Hq[i * 64 + lane] = o;
                    // base past the last bucket = number of non-NaN keys
                    if (i == QW - 1 && t == NT - 1) H[NB / 2] = base;
                }
            }
        }
        if (!go) {
            if (lo > hi) {
                // no value at this timepoint (every curve NaN): nothing is contained, nothing to rank
                if constexpr (J == 0) {
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        if (e < E - 1 || t + (E - 1) * NT < n) ABimg[r * n + t + e * NT] = AB_SPECIAL;
                    if (t == 0) nnan_img[r] = (u32)n;
                }
            } else {                                                  // set aside: sorted behind the loop
                if (t == 0) defer[rowidx >> 5] |= 1u << (rowidx & 31);
                ++ndefer;
            }
        }
        ++rowidx;
        u32 bc[E];                                                    // base | count << 16 | slot << 24; count 0: a NaN
        u32 (&pk)[E] = bs;                                            // member phase: less | le << 16, in bs's registers
        if (go) {
            __syncthreads();                                          // barrier 4
            // ---- (3) scatter into bucket order (branch-free; NaNs write the dummy slot) ----
            const u32 nv = H[NB / 2];
            nn = (u32)n - nv;
            if (!trypure) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const u32 b = bs[e] & 0xFFFFu, slot = bs[e] >> 16;
                    const u32 base = H16[b], end = H16[b + 1];
                    const bool isk = b < (u32)NB;
                    S[isk ? base + slot : (u32)DUMMY] = k[e];
                    bc[e] = isk ? (base | ((end - base) << 16) | (slot << 24)) : 0u;
                }
            } else {                                                  // counts and slots beyond 8 bits: two words
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const u32 b = bs[e] & 0xFFFFu, slot = bs[e] >> 16;
                    const u32 base = H16[b], end = H16[b + 1];
                    const bool isk = b < (u32)NB;
                    S[isk ? base + slot : (u32)DUMMY] = k[e];
                    bc[e] = base | (slot << 16);
                    pk[e] = isk ? end - base : 0u;
                }
            }
            if (nn && t < RB_PAD) S[nv + t] = QNAN;                   // sentinels behind a row shortened by NaNs
        }
        if (rnext < rows) load_row(rnext);                            // next row in flight under the member passes
        if (go) {
            __syncthreads();                                          // barrier 5
            // the histogram is dead until the next row's atomics (behind its barrier 1)
            {
                uint4 *Hq = reinterpret_cast<uint4 *>(H) + wave * (64 * QW);
#pragma unroll
                for (int i = 0; i < QW; ++i) Hq[i * 64 + lane] = make_uint4(0, 0, 0, 0);
            }
            // ---- (4) rank inside the bucket.  First pass, branch-free: 2*U2 keys from the even position at or
            //      below the bucket's base (16-byte reads); a key in front of an odd base belongs to an earlier
            //      bucket, compares below, and is taken off again.  Second pass: the rest of longer buckets. ----
            // A row with a bucket of 2^TRYB keys or more is tie-heavy data more often than a dense cluster: if every
            // bucket of the row holds ONE value (all members equal their bucket's first key), the ranks are closed
            // form -- less = 0, le = count -- and there is no member pass at all.  Else the row goes the normal way,
            // or to the sort behind the loop when a bucket is above CAP.
            int mode = 0;                                             // 0: member passes, 1: closed form, 2: set aside
            if (trypure) {                                            // block-uniform
                bool pure = true;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const u32 base = bc[e] & 0xFFFFu, slot = bc[e] >> 16;
                    if (pk[e]) pure = pure && (S[base + slot] == S[base]);
                }
                if (__syncthreads_and(pure)) {
                    mode = 1;
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const u32 cnt = pk[e];
                        bc[e] = (bc[e] & 0xFFFFu) | (cnt ? 0x10000u : 0u);
                        pk[e] = cnt << 16;
                    }
                } else if (crowded) {
                    mode = 2;
                    if (t == 0) defer[(rowidx - 1) >> 5] |= 1u << ((rowidx - 1) & 31);
                    ++ndefer;
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const u32 cnt = pk[e];
                        bc[e] = cnt ? ((bc[e] & 0xFFFFu) | (cnt << 16) | ((bc[e] >> 16) << 24)) : 0u;
                    }
                }
            }
            bool more = false;
            if (mode == 0) {
            // A key's window: its reads are issued together, ahead of the compares.  A lane whose bucket ends before
            // a pair reads the NaN pair behind the keys instead: same counts (NaN compares false), and lanes sharing
            // one address cost no bank-conflict cycles.  (Two windows in flight per lane: no faster, see DESIGN.)
            double xw[1];
            double2 yw[1][U2];
            auto window = [&](int e, int w) {
                const u32 base = bc[e] & 0xFFFFu, cnt = (bc[e] >> 16) & 0xFFu, slot = bc[e] >> 24;
                const u32 odd = base & 1u;
                xw[w] = S[base + slot];                               // own key (its registers hold the next row)
                const double2 *Sq = reinterpret_cast<const double2 *>(S + (base - odd));
#pragma unroll
                for (int u = 0; u < U2; ++u) {
                    yw[w][u] = *((u == 0 || cnt + odd > (u32)(2 * u)) ? Sq + u : NANP);
                }
            };
            window(0, 0);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int w = 0;
                const u32 base = bc[e] & 0xFFFFu, cnt = (bc[e] >> 16) & 0xFFu;
                const u32 odd = base & 1u;
                const double x = xw[w];
                u32 less = 0, le = 0;
#pragma unroll
                for (int u = 0; u < U2; ++u) {
                    less += (yw[w][u].x < x) ? 1u : 0u;
                    le += (yw[w][u].x <= x) ? 1u : 0u;
                    less += (yw[w][u].y < x) ? 1u : 0u;
                    le += (yw[w][u].y <= x) ? 1u : 0u;
                }
                pk[e] = (less - odd) | ((le - odd) << 16);
                more |= cnt + odd > (u32)(2 * U2);
                if (e + 1 < E) window(e + 1, 0);
            }
            if (__ballot(more) != 0) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    u32 bce = bc[e];
                    asm volatile("" : "+v"(bce));                     // unpack again here: nothing kept alive from pass 1
                    const u32 base = bce & 0xFFFFu, cnt = (bce >> 16) & 0xFFu, slot = bce >> 24;
                    const u32 odd = base & 1u;
                    if (cnt + odd > (u32)(2 * U2)) {
                        const double x = S[base + slot];
                        const double2 *Sq = reinterpret_cast<const double2 *>(S + (base - odd));
                        u32 less = 0, le = 0;
#pragma unroll 1
                        for (u32 kk = 2 * U2; kk < cnt + odd; kk += 2) {
                            const double2 y = Sq[kk >> 1];
                            less += (y.x < x) ? 1u : 0u;
                            le += (y.x <= x) ? 1u : 0u;
                            less += (y.y < x) ? 1u : 0u;
                            le += (y.y <= x) ? 1u : 0u;
                        }
                        pk[e] += less | (le << 16);
                    }
                }
            }
            }                                                         // mode == 0
            // ---- fold ----
            if (mode != 2) {
            const u32 nv = (u32)n - nn;                               // non-NaN keys of the row
            const u32 v = nv - 1u;                                    // valid others of a non-NaN target
            const u32 R2 = v * (v - 1u + 2u * nn);                    // J == 2: 2 * [N v + C(v,2)]  (< 2^30)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const u32 base = bc[e] & 0xFFFFu, cnt = (bc[e] >> 16) & 0xFFu;
                const u32 B = base + (pk[e] & 0xFFFFu), A = nv - base - (pk[e] >> 16);
                if constexpr (J == 0) {
                    if (e < E - 1 || t + (E - 1) * NT < n) ABimg[r * n + t + e * NT] = cnt ? (B | (A << 16)) : AB_SPECIAL;
                } else if constexpr (J == 2) {
                    // 2 * contained_2 = 2 N (v - A - B) + v(v-1) - A(A-1) - B(B-1)   (all terms < 2^30)
                    u32 q = __umul24(A, A - 1u) + __umul24(B, B - 1u);   // A, B < 2^15: 24-bit multiplies are exact
                    if (nn) q += 2u * __umul24(nn, A + B);
                    acc[e][0] += (ACC)(cnt ? R2 - q : 0u);
                } else {
                    if (cnt) {
                        u64 a7[JMAX - 1] = {0, 0, 0, 0, 0, 0, 0};
                        band_counts_add<(J > 0 ? J : 2)>(A, B, nn, (u64)(n - 1), a7);
#pragma unroll
                        for (int j = 0; j < J - 1; ++j) acc[e][j] += a7[j];
                    }
                }
            }
            }                                                         // mode != 2
        }
        if constexpr (J == 0) {
            if (go && t == 0) nnan_img[r] = nn;
        }
        if (rnext < rows) row_range(par);                             // the next row's keys have landed by now
    }
    t = t0;
    // ---- this workgroup's partial totals (u32 when the host found that they fit: J = 2, few rows per workgroup) ----
    u64 *P = partial + (size_t)blockIdx.x * (J > 0 ? J - 1 : 0) * n;
    // SEL: the totals of the flagged rows go to this workgroup's own u32 block (summed by the last workgroups to arrive, below)
    u32 *P32 = SEL ? fblocks + (size_t)blockIdx.x * ((n + 3) & ~3) : reinterpret_cast<u32 *>(partial) + (size_t)blockIdx.x * n;
#pragma unroll
    for (int e = 0; e < E; ++e)
        if ((J > 0) && (e < E - 1 || t + (E - 1) * NT < n)) {
            if constexpr (J == 2) {
                if constexpr (SEL) { if ((i64)blockIdx.x < rows) P32[t + e * NT] = (u32)(acc[e][0] >> 1); }   // (else: never read)
                else if (p32) P32[t + e * NT] = (u32)(acc[e][0] >> 1);
                else P[t + e * NT] = acc[e][0] >> 1;
            } else {
#pragma unroll
                for (int j = 0; j < J - 1; ++j) P[(size_t)j * n + t + e * NT] = acc[e][j];
            }
        }
    // ---- the rows the bucket map could not spread (an infinity, all values equal, a crowded bucket): sort + search.
    //      The main loop's accumulators are already in HBM and dead here, so this cold code shares no registers
    //      with the hot loop; each thread adds its own curves' band counts to what it stored above. ----
    if (ndefer) {                                                     // block-uniform
        __syncthreads();
        rowidx = 0;
        for (i64 r = blockIdx.x; r < rows; r += gridDim.x, ++rowidx) {
            if (!((defer[rowidx >> 5] >> (rowidx & 31)) & 1u)) continue;
            u32 ab[RB_SE], nnan_s;
            rb_slow_row(rowptr(r), n, IMG, wtot, ab, &nnan_s);
#pragma unroll 1
            for (int e = 0; e < RB_SE; ++e) {
                if constexpr (J == 0) {
                    if (t + e * NT < n) ABimg[r * n + t + e * NT] = ab[e];
                    if (e == 0 && t == 0) nnan_img[r] = nnan_s;
                } else if (ab[e] != AB_SPECIAL) {                         // implies t + e * NT < n
                    u64 a7[JMAX - 1] = {0, 0, 0, 0, 0, 0, 0};
                    band_counts_add<(J > 0 ? J : 2)>(ab[e] >> 16, ab[e] & 0xFFFFu, nnan_s, (u64)(n - 1), a7);
                    if (SEL || (J == 2 && p32)) P32[t + e * NT] += (u32)a7[0];
                    else {
#pragma unroll
                        for (int j = 0; j < J - 1; ++j) P[(size_t)j * n + t + e * NT] += a7[j];
                    }
                }
            }
        }
    }
    if constexpr (SEL) {
        // ---- the flagged rows' totals: G blocks of u32 -> out_tot.  Adding them with atomics from every workgroup costs
        //      G same-address atomics per curve (20 us at G = 256); instead each workgroup publishes its block, takes a
        //      ticket, and the LAST K workgroups to arrive each sum one slice of the curves over all blocks.  A waiting
        //      workgroup holds its CU, so the wait ends only if the workgroups that have not started yet still find one: the
        //      host passes K = kspin <= (workgroups the launch's CUs hold at once) - 1 (launch_bucket_sel_cfg: occupancy x the
        //      stream's CU mask; every workgroup resident at once: 16), and K = 1 never waits. ----
        const int G = (int)gridDim.x, K = G < kspin ? G : (kspin < 1 ? 1 : kspin);
        const int Gs = rows < (i64)G ? (int)rows : G;                 // workgroups that had a flagged row: the others' blocks are not read
        __syncthreads();                                              // this workgroup's block is complete (stores acknowledged) ...
        if (t0 == 0) {
            __threadfence();                                          // ... and written back for the device (ONE fence per workgroup)
            const u32 ticket = atomicAdd(done, 1u);                   // *done was zeroed by rank_bucket32_kernel
            wtot[0] = ticket;
            if (ticket >= (u32)(G - K))
                while (__hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (u32)G) __builtin_amdgcn_s_sleep(8);
            __threadfence();                                          // acquire: the other workgroups' blocks
        }
        __syncthreads();
        const u32 ticket = wtot[0];
        if (ticket < (u32)(G - K)) return;
        const int my = (int)ticket - (G - K);
        u64 *redl = reinterpret_cast<u64 *>(Sm);                      // [16 slices][64 quads][4]
        const int nst = (n + 3) & ~3, nq = nst >> 2;
        const int q0 = (int)((i64)my * nq / K), q1 = (int)((i64)(my + 1) * nq / K);
        const int qx = t0 & 63, y = t0 >> 6;
        for (int qb = q0; qb < q1; qb += 64) {
            u64 a0 = 0, a1 = 0, a2 = 0, a3 = 0;
            if (qb + qx < q1) {
                const u32 *pp = fblocks + 4 * (qb + qx);
#pragma unroll 8
                for (int g = y; g < Gs; g += 16) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(pp + (size_t)g * nst);
                    a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
                }
            }
            u64 *rl = redl + ((size_t)y * 64 + qx) * 4;
            rl[0] = a0; rl[1] = a1; rl[2] = a2; rl[3] = a3;
            __syncthreads();
            if (t0 < 256 && qb + (t0 >> 2) < q1 && 4 * (qb + (t0 >> 2)) + (t0 & 3) < n) {
                u64 tot = 0;
#pragma unroll
                for (int k = 0; k < 16; ++k) tot += redl[((size_t)k * 64 + (t0 >> 2)) * 4 + (t0 & 3)];
                atomicAdd(&out_tot[4 * (qb + (t0 >> 2)) + (t0 & 3)], tot);
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Z: out[q][j] (+)= sum_g partial[g][j][i(q)] + fold of the pair-image rows flagged in rowflag.
// block = 32 targets x 32 slices (of workgroups g, of rows), LDS tree over the slices.  rowflag == nullptr: no pair image
// (the bucket kernel ranks every row itself).
// ---------------------------------------------------------------------------------------------------
template <int J>
__global__ __launch_bounds__(1024) void rank_finalize_kernel(const u64 *__restrict__ partial, int G, int p32,
                                                             const u32 *__restrict__ AB, const u32 *__restrict__ nnan,
                                                             const unsigned char *__restrict__ rowflag, i64 rows, i64 n,
                                                             const i64 *__restrict__ targets, i64 tbegin, i64 m,
                                                             u64 *__restrict__ out, int first) {
    __shared__ u64 red[32][33];
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
    const i64 q = (i64)blockIdx.x * 32 + x;
    const i64 i = (q < m) ? (targets ? targets[q] : tbegin + q) : 0;
    // any deferred row at all?  (one pass over the flags by the whole block; normally none)
    int any = 0;
    if (rowflag) {                                                    // block-uniform
        for (i64 r = threadIdx.x; r < rows; r += 1024) any |= rowflag[r];
        any = __syncthreads_or(any);
    }
    u64 acc[JMAX - 1];
#pragma unroll
    for (int j = 0; j < JMAX - 1; ++j) acc[j] = 0;
    if (q < m) {
        if (J == 2 && p32) {
            const u32 *p = reinterpret_cast<const u32 *>(partial) + i;
#pragma unroll 8
            for (int g = y; g < G; g += 32) acc[0] += p[(size_t)g * n];
        } else {
            const u64 *p = partial + i;
#pragma unroll 8
            for (int g = y; g < G; g += 32) {
#pragma unroll
                for (int j = 0; j < J - 1; ++j) acc[j] += p[((size_t)g * (J - 1) + j) * n];
            }
        }
        if (any) {
            for (i64 r = y; r < rows; r += 32) {
                if (rowflag[r]) fold_pair16<J>(AB[r * n + i], nnan[r], n, acc);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < J - 1; ++j) fold_store(red, x, y, acc[j], q < m, out + q * (J - 1) + j, first);
}

// Z for the common case (J = 2, u32 partial totals, a contiguous 4-aligned block of targets, no pair image): thread
// (x, y) of a 256-thread block sums slice y of the G partial blocks for the 4 curves tbegin + 4 (8 blockIdx + x) ..
// with 16-byte loads; block = 32 curves x 32 slices.
__global__ __launch_bounds__(256) void rank_finalize4_kernel(const u32 *__restrict__ partial, int G, i64 n, i64 tbegin, i64 m,
                                                            u64 *__restrict__ out, int first) {
    __shared__ u64 red[32][8][4 + 1];
    const int x = threadIdx.x & 7, y = threadIdx.x >> 3;
    const i64 q = ((i64)blockIdx.x * 8 + x) * 4;                      // first of this thread's 4 targets
    u64 a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    if (q < m) {
        const u32 *p = partial + tbegin + q;
#pragma unroll 8
        for (int g = y; g < G; g += 32) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p + (size_t)g * n);
            a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
        }
    }
    const u64 a[4] = {a0, a1, a2, a3};
    fold_store_w<32, 8, 4, 5, 8 * 5>(&red[0][0][0], x, y, a, (i64)blockIdx.x * 32, m, out, 1, first);
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
// the workgroups' partial totals: all this path keeps in HBM (2 * CUs: the upper bound of the grid the launchers use)
size_t mbd_rank_bucket_partial_bytes(i64 n, int J) { return align_up((size_t)2 * device_cus() * (J - 1) * n * 8, 256); }

constexpr int RB_CAP = 127;
template <int NT, int E, int LNB, int J, int U2>
static int launch_bucket_cfg(const double *Y, i64 n, i64 row0, i64 rows, u64 *partial, int p32, int G, hipStream_t s,
                             u32 *nnan_img = nullptr) {
    using C = RBCfg<NT, E, LNB, U2>;
    auto kf = rank_bucket_kernel<NT, E, LNB, J, RB_CAP, U2>;
    if constexpr (J == 2) {
        if (p32 == RB_PARTIAL_ACC32) kf = rank_bucket_kernel<NT, E, LNB, J, RB_CAP, U2, true>;
    }
    const size_t lds = C::lds_bytes((int)n);
    if (lds > 163840) return fail(SD_ERR_UNSUPPORTED, "bucket kernel: %zu bytes of LDS for n=%lld", lds, (long long)n);
    return rb_launch(kf, G, NT, lds, s, Y, n, row0, rows, partial, p32, nnan_img, nullptr, nullptr, 0u, nullptr, 0, nullptr, nullptr, 1);
}

// second launch behind rank_bucket32_kernel: the rows it flagged, totals added to its partial blocks
template <int E, int LNB>
static int launch_bucket_sel_cfg(const double *Y, i64 n, i64 row0, i64 rows, u64 *partial, int G, const unsigned char *rowflag,
                                 const u32 *gate, u32 epoch, u64 *out, int Gsum, u32 *fblocks, u32 *done,
                                 hipStream_t s) {
    using C = RBCfg<1024, E, LNB, 3>;
    auto kf = rank_bucket_kernel<1024, E, LNB, 2, RB_CAP, 3, true, true>;
    const size_t lds = C::lds_bytes((int)n) + 8192;
    if (lds > 163840) return fail(SD_ERR_UNSUPPORTED, "bucket kernel: %zu bytes of LDS for n=%lld", lds, (long long)n);
    // workgroups that may wait for the others at the end of the kernel: fewer than the launch's CUs hold at once
    int kspin = 1;
    {
        static int occ_cached = 0;                            // per instantiation (benign race: same value)
        int occ = occ_cached;
        if (occ <= 0) {                                       // (asked once, with the kernel's LDS limit raised as for the launch)
            SD_HIP(hipFuncSetAttribute((const void *)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)kf, 1024, lds) != hipSuccess || occ < 1) occ = 1;
            occ_cached = occ;
        }
        const int usable = stream_cus(s);
        const bool masked = usable < device_cus();
        const long cap = (long)occ * usable;
        kspin = cap >= G ? 16 : (int)(cap - 1 < 16 ? cap - 1 : 16);
        // A masked stream: the launch's CUs are not one pool.  Workgroups are dealt to the 8 XCDs in turn and stay there, so a
        // waiter on an XCD that the mask left one CU starves that XCD's remaining workgroups however many CUs the others have
        // free (found with tools/cu_mask_check.py: 8 CUs, one per XCD, 7 waiters -- the kernel never ended).  K = 1 never waits.
        if (masked) kspin = 1;
        if (kspin < 1) kspin = 1;
    }
    return rb_launch(kf, G, 1024, lds, s, Y, n, row0, rows, partial, RB_PARTIAL_ACC32, nullptr, rowflag, gate, epoch, out, Gsum, fblocks,
                     done, kspin);
}

// fold (J = 2, 3) and image mode (J = 0, partial = the image, nnan_img = its NaN counts); first member pass: 3 x 16 bytes
template <int J>
static int launch_bucket_e(const double *Y, i64 n, i64 row0, i64 rows, u64 *partial, int p32, int G, hipStream_t s,
                           u32 *nnan_img = nullptr) {
#define RB_E(E_) case E_: return launch_bucket_cfg<1024, E_, rb_lnb(E_, J), J, 3>(Y, n, row0, rows, partial, p32, G, s, nnan_img);
    switch ((int)((n + 1023) / 1024)) {
        RB_E(1) RB_E(2) RB_E(3) RB_E(4) RB_E(5) RB_E(6) RB_E(7) RB_E(8) RB_E(9) RB_E(10) RB_E(11) RB_E(12) RB_E(13) RB_E(14)
        RB_E(15) RB_E(16)
    }
#undef RB_E
    return fail(SD_ERR_UNSUPPORTED, "bucket kernel covers n <= 16384");
}

// image mode (J >= 4 on the host side): pairs of every (row, curve) to AB, NaN counts per row to nnan
int launch_rank_bucket_image(const double *Y, i64 n, i64 row0, i64 rows, u32 *AB, u32 *nnan, hipStream_t s) {
    const int cus = device_cus();
    const int G = (int)(rows < cus ? rows : cus);
    if (rows > (i64)G * 2048) return fail(SD_ERR_INVALID, "bucket kernel: more than 2048 rows per workgroup in one launch");
    return launch_bucket_e<0>(Y, n, row0, rows, reinterpret_cast<u64 *>(AB), RB_PARTIAL_U64, G, s, nnan);
}

// J = 2, 4096 < n <= 11264, every curve a target: rank_bucket32_kernel (two workgroups per CU; zeroes out when `first`) + the
// fp64 kernel's SEL form (sums the partial blocks into out; ranks the rows the first kernel flagged).  Two launches.  The
// flags and the gate word sit behind the 2 * cus u32 partial blocks, inside the space sized for u64 blocks.
// what the two-launch path carves out of the partial-block space: its u32 blocks, row flags, gate words, the second
// launch's blocks -- and, last, n u64 totals of ALL curves for calls that ask for a subset of the targets
static size_t two_level_used_bytes(i64 n, i64 rows) {
    const size_t pst = (size_t)((n + 31) & ~31), nst = (size_t)((n + 3) & ~3);
    return (size_t)2 * device_cus() * pst * 4 + align_up((size_t)rows, 64) + 64 + 256 +
           (size_t)device_cus() * nst * 4 + 256;
}
bool rank_bucket_two_level_supported(i64 n, i64 rows) {
    // the all-totals block sits behind the largest batch's region (rank_bucket_two_level_all_totals): the same expression here
    return rank_bucket32_supported(n, rows, device_cus()) &&
           align_up(two_level_used_bytes(n, 4096), 256) + (size_t)n * 8 <= mbd_rank_bucket_partial_bytes(n, 2);
}
u64 *rank_bucket_two_level_all_totals(u64 *partial, i64 n) {        // sized for the largest batch (4 096 rows)
    return reinterpret_cast<u64 *>(reinterpret_cast<char *>(partial) + align_up(two_level_used_bytes(n, 4096), 256));
}

// out[q] (=|+=) all[target q]: the subset of the totals a call asked for
__global__ __launch_bounds__(256) void rank_gather_totals_kernel(const u64 *__restrict__ all, const i64 *__restrict__ targets, i64 tbegin,
                                                                i64 m, u64 *__restrict__ out) {
    const i64 q = (i64)blockIdx.x * 256 + threadIdx.x;
    if (q < m) out[q] = all[targets ? targets[q] : tbegin + q];
}
int launch_rank_gather_totals(const u64 *all, const i64 *targets, i64 tbegin, i64 m, u64 *out, hipStream_t s) {
    hipLaunchKernelGGL(rank_gather_totals_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, all, targets, tbegin, m, out);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

int launch_rank_bucket_two_level(const double *Y, i64 n, i64 row0, i64 rows, u64 *partial, u64 *out, int first, hipStream_t s) {
    const int cus = device_cus();
    const int G = (int)(rows < 2 * cus ? rows : 2 * cus);
    u32 *P32 = reinterpret_cast<u32 *>(partial);
    unsigned char *rowflag = reinterpret_cast<unsigned char *>(P32 + (size_t)2 * cus * ((n + 31) & ~31));   // blocks of whole lines
    u32 *gate = reinterpret_cast<u32 *>(rowflag + align_up((size_t)rows, 64));
    // the second launch's own blocks (totals of the flagged rows), 16-byte aligned, behind the gate words; gate[2]: arrival counter
    u32 *fblocks = reinterpret_cast<u32 *>(align_up((size_t)(gate + 16), 256));
    const u32 epoch = rank_bucket32_epoch();
    int rc = launch_rank_bucket32(Y, n, row0, rows, P32, rowflag, gate, epoch, first ? out : nullptr, G, s);
    if (rc) return rc;
    const int G2 = G < cus ? G : cus;
    // a table of its own, not rb_lnb: the SEL form takes 16384 buckets at E = 3, 4 and 11 too (32768 at E = 10 only)
#define RB_SEL(E_) case E_: return launch_bucket_sel_cfg<E_, 14>(Y, n, row0, rows, partial, G2, rowflag, gate, epoch, out, G, fblocks, gate + 2, s);
    switch ((int)((n + 1023) / 1024)) {
        RB_SEL(3) RB_SEL(4) RB_SEL(5) RB_SEL(6) RB_SEL(7) RB_SEL(8) RB_SEL(9) RB_SEL(11)
        case 10: return launch_bucket_sel_cfg<10, 15>(Y, n, row0, rows, partial, G2, rowflag, gate, epoch, out, G, fblocks, gate + 2, s);
    }
#undef RB_SEL
    return fail(SD_ERR_UNSUPPORTED, "two-level bucket path covers 4096 < n <= 11264");
}

// rows [row0, row0 + rows): partial totals of every curve per workgroup; returns the grid used (number of partial
// blocks) in *G_out
int launch_rank_bucket(const double *Y, i64 n, i64 row0, i64 rows, int J, u64 *partial, int *p32_out, int *G_out,
                       hipStream_t s) {
    const int cus = device_cus();                                         // one workgroup per CU
    const int G = (int)(rows < cus ? rows : cus);
    *G_out = G;
    if (rows > (i64)G * 2048) return fail(SD_ERR_INVALID, "bucket kernel: more than 2048 rows per workgroup in one launch");
    // J = 2: a workgroup's total is at most ceil(rows / G) * C(n-1, 2); below 2^32 the partials travel as u32
    const u64 per_wg = (u64)((rows + G - 1) / G) * ((u64)(n - 1) * (u64)(n - 2) / 2);
    int p32 = (J == 2 && per_wg < ((u64)1 << 32)) ? RB_PARTIAL_U32 : RB_PARTIAL_U64;
    // ... and 2 * total stays below 2^32 too (2 * C(v,2) + 2 N v < n^2 per row): the kernel accumulates in 32 bits
    if (p32 && (u64)((rows + G - 1) / G) * (u64)n * (u64)n < ((u64)1 << 32) && xswitch("SD_RB_ACC64") == 0) p32 = RB_PARTIAL_ACC32;
    *p32_out = p32;
    if (J == 2) return launch_bucket_e<2>(Y, n, row0, rows, partial, p32, G, s);
    if (J == 3) return launch_bucket_e<3>(Y, n, row0, rows, partial, p32, G, s);
    return fail(SD_ERR_UNSUPPORTED, "bucket kernel covers J in [2,3]");
}

int launch_rank_finalize(const u64 *partial, int G, int p32, const u32 *AB, const u32 *nnan, const unsigned char *rowflag,
                         i64 rows, i64 n, const i64 *targets, i64 tbegin, i64 m, int J, u64 *out, int first,
                         hipStream_t s) {
    dim3 grid((unsigned)((m + 31) / 32));
    if (J == 2 && p32 && !targets && !rowflag && n % 4 == 0 && tbegin % 4 == 0 && m % 4 == 0 && xswitch("SD_RB_FINAL1") == 0)
        hipLaunchKernelGGL(rank_finalize4_kernel, grid, dim3(256), 0, s, reinterpret_cast<const u32 *>(partial), G, n, tbegin, m,
                           out, first);
    else if (J == 2)
        hipLaunchKernelGGL((rank_finalize_kernel<2>), grid, dim3(1024), 0, s, partial, G, p32, AB, nnan, rowflag, rows, n, targets,
                           tbegin, m, out, first);
    else
        hipLaunchKernelGGL((rank_finalize_kernel<3>), grid, dim3(1024), 0, s, partial, G, p32, AB, nnan, rowflag, rows, n, targets,
                           tbegin, m, out, first);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

}  // namespace sd
