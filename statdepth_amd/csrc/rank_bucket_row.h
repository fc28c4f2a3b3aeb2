// rank_bucket_row.h -- what the fp64 bucket kernels share beyond rank_bucket.h's cross-lane helpers (internal): the LDS layout
// of a row (RBCfg), the bucket count per row width (rb_lnb), their launch, and RbRow, the per-row bucket build of
// rank_external_kernel (mbd_rank_external.hip) and rank_medium_image_kernel (mbd_rank_medium.hip).  rank_bucket_kernel
// (mbd_rank_bucket.hip) takes the layout and the launch from here and spells out its own variant of the build: packed
// addition in the prefix sum, the CAP / TRYB flags, the next row's range behind the member passes.
#pragma once
#include "rank_bucket.h"

namespace sd {

// Rows whose range is much wider than their bulk (heavy tails, outlying curves): the three-piece map of rank_bucket.h.  Rounds
// 1 - 3 clamped the tails into the two end buckets of a range clipped to the waves' innermost extremes: three outlying curves
// were fine, heavy tails at every timepoint set every row aside for the sort (n = 14 000 Cauchy rows: 3.4 x the Gaussian time).
constexpr int RB_PAD = 8;                      // NaN sentinels behind the bucket-ordered keys (never < or <= anything)
constexpr int RB_SNT = 1024, RB_SE = 16;       // rb_slow_row (mbd_rank_bucket.hip): threads, keys per thread

template <int NT, int E, int LNB, int U2>
struct RBCfg {
    static constexpr int NB = 1 << LNB;
    static constexpr int NW = NT / 64;
    static constexpr int W = NB / 2 / NT;                       // histogram words per thread in the prefix sum
    static constexpr int QW = W / 4;                            // ... as 16-byte quads
    static_assert(W >= 4 && W % 4 == 0, "whole quads of histogram words per thread");
    static_assert(NW == 16 || NW == 8, "cross-wave reductions are laid out for rows of 16 lanes");
    static_assert(NT == RB_SNT, "rb_slow_row is compiled for 1024 threads");
    // positions: [0, n) keys, [n, n + RB_PAD) sentinels, DUMMY.. a scratch pair range for keys that are NaN
    static __host__ __device__ constexpr int dummy_pos(int n) { return (n + RB_PAD + 1) & ~1; }
    static __host__ __device__ constexpr size_t keys_slots(int n) { return (size_t)dummy_pos(n) + 2 * U2 + 2; }
    static constexpr int DEFW = 64;                              // bitmap of set-aside rows: 2048 rows per workgroup and launch
    // min/max partials, wave totals, bitmap, 64 spare bytes, the waves' brackets ([3][NW] float2: rb3_wave_bracket)
    static constexpr size_t HDR = (size_t)4 * NW * 8 + (size_t)NW * 4 + (size_t)DEFW * 4 + 64 + (size_t)6 * NW * 4;
    static constexpr int BRK_WORD = NW + DEFW + 16;                // of the brackets, in u32 words behind the min/max partials
    static __host__ __device__ constexpr size_t lds_bytes(int n) {
        const size_t a = keys_slots(n) * 8 + (size_t)(NB / 2 + 4) * 4;
        const size_t n_act = (size_t)((n + 1023) / 1024) * 1024;
        const size_t b = (n_act + n_act / 16) * 8;                  // sort image of rb_slow_row (R2Cfg<1024,16> slots)
        return HDR + (a > b ? a : b);
    }
};

// log2 of the buckets for E = ceil(n / 1024) keys per thread, J = 2, 3 or 0 (the pair-image mode): 8192 buckets up to n = 4096,
// 16384 above while keys + histogram fit the 160 KiB of LDS (8192 at E = 16), 32768 at E = 10, 11 for J = 2 and the pair-image
// mode (measured: -2..-3.5 % on continuous rows, -7 % with outlying curves, +6 % on tie-heavy rows whose closed form only
// pays the longer prefix sum; J = 3 stays at 16384: the wider prefix arrays push it further into scratch).  The external and
// the medium kernel take the J = 3 column.
constexpr int rb_lnb(int E, int J) { return (E <= 4 || E == 16) ? 13 : ((E == 10 || E == 11) && J != 3) ? 15 : 14; }

// one launch of a kernel that takes `lds` bytes of dynamic LDS (above the 64 KiB a kernel gets unasked)
template <class... P, class... A>
static int rb_launch(void (*kf)(P...), int G, int NT, size_t lds, hipStream_t s, A... args) {
    SD_HIP(hipFuncSetAttribute((const void *)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kf, dim3(G), dim3(NT), lds, s, static_cast<P>(args)...);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

#ifdef __HIPCC__
// ---------------------------------------------------------------------------------------------------
// The bucket build of one row (or one column block of a row) of at most E * NT keys, phases (0) - (3) of the kernels' headers:
// (0) range, (1) bucket + slot from one LDS atomic per key, (2) exclusive prefix sum of the counters into packed
// `base | end << 16` words, (3) keys scattered into bucket order.  Afterwards bucket b holds S[H16[b] .. H16[b + 1]), and
// the bucket_of() of what build() returned -- the map the row was BUILT with, the only one there is for a look-up -- names the
// bucket of any value.
//   CROWD  a bucket of 2^CROWD keys or more makes the row `trypure`: tie-heavy data, or a range much wider than the row's bulk.
//          The central bracket tells them apart; the second kind is histogrammed again under the three-piece map (rank_bucket.h),
//          and the rows behind it (`heavy`) take their bracket with their range, before the histogram.
//   FLAT   infinite keys stay out of the range (they take the end buckets anyway), and a row whose finite keys hold one value
//          (`flat`) takes neither bracket nor clip: its look-ups need no map.
// One object per workgroup and launch; every branch around a barrier is block-uniform.
// ---------------------------------------------------------------------------------------------------
template <int NT, int E, int LNB, int CROWD, bool FLAT>
struct RbRow {
    using C = RBCfg<NT, E, LNB, 3>;
    static constexpr int NB = C::NB, NW = C::NW, QW = C::QW;
    double *red;                                                      // [2][NW][2] min/max partials
    u32 *wtot;                                                        // [NW]
    float2 *brk;                                                      // [NW] the waves' brackets
    u32 *H;                                                           // NB packed u16 counters, then bases
    double *S;                                                        // keys in bucket order
    const unsigned short *H16;
    int t, lane, wave;                                                // thread(): once per row
    int par = 0;
    bool heavy = false;                                               // block-uniform: the last build went under the three-piece map
    // What build() returns: the map the keys were placed with, and what the row turned out to be.  All but bs block-uniform.
    struct Built {
        double lo, hi, scale;                                         // the linear map ...
        Rb3 m3;                                                       // ... or, m3.clip, the three-piece one
        bool flat, trypure;
        u32 nv;                                                       // keys that are not NaN
        u32 bs[E];                                                    // bucket | slot << 16 of this thread's keys; NaN: bucket NB + 2
        __device__ __forceinline__ u32 bucket_of(double x) const { return bucket(m3, lo, scale, x); }
    };
    static __device__ __forceinline__ u32 bucket(const Rb3 &m3, double lo, double scale, double x) {
        if (m3.clip) return rb3_bucket<NB>(m3, x);                    // block-uniform
        double u = (x - lo) * scale;
        u = u > 0.0 ? u : 0.0;                                        // below the range, and NaN (0 * inf) -> 0
        u = u < (double)(NB - 1) ? u : (double)(NB - 1);
        return (u32)u;
    }

    // the workgroup's LDS; leaves the histogram empty (a barrier follows in build())
    __device__ __forceinline__ explicit RbRow(double *Sm) {
        red = Sm;
        wtot = reinterpret_cast<u32 *>(red + 4 * NW);
        brk = reinterpret_cast<float2 *>(wtot + C::BRK_WORD);
        H = reinterpret_cast<u32 *>(Sm + C::HDR / 8);
        S = reinterpret_cast<double *>(H + NB / 2 + 4);
        H16 = reinterpret_cast<const unsigned short *>(H);
        uint4 *Hq = reinterpret_cast<uint4 *>(H);
#pragma unroll
        for (int i = 0; i < QW; ++i) Hq[i * NT + threadIdx.x] = make_uint4(0, 0, 0, 0);
        if (threadIdx.x < 4) H[NB / 2 + threadIdx.x] = 0;
    }
    // the kernel's per-row opaque copy of the thread id (see rank_bucket_kernel)
    __device__ __forceinline__ void thread(int t_) {
        t = t_;
        lane = t & 63;
        wave = __builtin_amdgcn_readfirstlane(t >> 6);
    }
    // this wave's 64 * QW quads of the histogram, quad i * 64 + lane (conflict-free 16-byte accesses: lane <-> quad)
    __device__ __forceinline__ uint4 *quads() const { return reinterpret_cast<uint4 *>(H) + wave * (64 * QW); }
    // the histogram is dead from the barrier behind the last look-up until the next build's atomics (behind its barrier 1)
    __device__ __forceinline__ void clear() const {
        uint4 *Hq = quads();
#pragma unroll
        for (int i = 0; i < QW; ++i) Hq[i * 64 + lane] = make_uint4(0, 0, 0, 0);
    }
    // k: this thread's keys (NaN where it has none); nkeys: keys of the row, for the map's crowding estimate; dummy: the
    // position behind the sentinels where NaN keys land.  Barriers 1 - 4 of the kernels; the caller's barrier 5 ends the scatter.
    __device__ __forceinline__ Built build(const double (&k)[E], int nkeys, int dummy) {
        const double INF = __builtin_huge_val();
        Built b;
        Rb3 &m3 = b.m3;
        // ---- (0) range ----
        // (the first step through the builtins, whose infinite seeds are scalar operands: rb_mm's inline assembly would hold them
        // in two VGPR pairs across the whole row loop)
        double mn, mx;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const double xf = (FLAT && (k[e] == INF || k[e] == -INF)) ? __builtin_nan("") : k[e];
            mn = e ? rb_mm<false>(mn, xf) : __builtin_fmin(INF, xf);
            mx = e ? rb_mm<true>(mx, xf) : __builtin_fmax(-INF, xf);
        }
        const double tmn = mn, tmx = mx;                              // this thread's own extremes (the bracket's groups)
        mn = rb_wave_allreduce<false>(mn);
        mx = rb_wave_allreduce<true>(mx);
        double *redp = red + par * 2 * NW;
        if (lane == 63) { redp[2 * wave] = mn; redp[2 * wave + 1] = mx; }
        par ^= 1;
        __syncthreads();                                              // barrier 1
        m3.clip = false;
        double lo, hi;
        {
            const double2 p = reinterpret_cast<const double2 *>(redp)[lane & (NW - 1)];
            lo = rb_readlane_f64(rb_row_allreduce<false>(p.x), 0);
            hi = rb_readlane_f64(rb_row_allreduce<true>(p.y), 0);
        }
        const bool flat = FLAT && hi == lo;                                     // every finite key holds one value
        double scale = (double)NB / (hi - lo);
        // equal values, an infinity in the range, a range too small or too large: everything into one bucket
        if (!((hi > lo) && (scale < INF) && (lo > -INF) && (hi < INF))) scale = 0.0;
        // ---- (1) histogram ----
        auto bracket_map = [&]() -> Rb3 {
            const float2 wb = rb3_wave_bracket<E, NT>(tmn, tmx);
            if (lane == 63) brk[wave] = wb;
            __syncthreads();
            return rb3_make<NB>(lo, hi, brk[lane & (NW - 1)], nkeys);
        };
        if (heavy && !flat) {                                         // block-uniform: the last build went under core + tails
            m3 = bracket_map();
            heavy = m3.clip;
        }
        auto histogram = [&]() {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double x = k[e];
                u32 bk = bucket(m3, lo, scale, x);
                bk = (x == x) ? bk : (u32)(NB + 2);                   // NaNs count into a dummy word behind the histogram
                const u32 sh = (bk & 1u) * 16u;
                const u32 old = atomicAdd(&H[bk >> 1], 1u << sh);
                b.bs[e] = bk | (((old >> sh) & 0xFFFFu) << 16);
            }
        };
        histogram();
        __syncthreads();                                              // barrier 2
        // ---- (2) exclusive prefix sum ----
        uint4 *Hq = quads();
        uint4 hq[QW];
        u32 runq[QW], inclq[QW], offq[QW];
        auto prefix_a = [&]() {
            u32 wsum = 0, ov = 0;
#pragma unroll
            for (int i = 0; i < QW; ++i) {
                hq[i] = Hq[i * 64 + lane];
                const u32 lo16 = (hq[i].x & 0xFFFFu) + (hq[i].y & 0xFFFFu) + (hq[i].z & 0xFFFFu) + (hq[i].w & 0xFFFFu);
                const u32 hi16 = (hq[i].x >> 16) + (hq[i].y >> 16) + (hq[i].z >> 16) + (hq[i].w >> 16);
                ov |= hq[i].x | hq[i].y | hq[i].z | hq[i].w;          // bit k of a half set <=> some counter has it
                runq[i] = lo16 + hi16;                                // counters reach the key count here: no packed addition
                inclq[i] = rb_wave_incl_scan(runq[i]);
                offq[i] = wsum;
                wsum += rb_readlane(inclq[i], 63);
            }
            constexpr u32 TRM = (0xFFFFu & ~((1u << CROWD) - 1u)) * 0x10001u;   // some counter >= 2^CROWD: a bit from there up is set
            const bool wtry = __ballot((ov & TRM) != 0) != 0;
            if (lane == 63) wtot[wave] = wsum | (wtry ? 0x40000000u : 0u);
        };
        prefix_a();
        __syncthreads();                                              // barrier 3
        u32 wt = wtot[lane & (NW - 1)];
        bool trypure = __ballot((wt & 0x40000000u) != 0) != 0;
        if (trypure && !flat && !m3.clip) {                           // block-uniform, rare: ties -- or a range much wider than
            m3 = bracket_map();                                       // the bulk (see rank_bucket_kernel): again under core + tails
            if (m3.clip) {
                heavy = true;
                clear();
                if (t < 4) H[NB / 2 + t] = 0;
                __syncthreads();
                histogram();
                __syncthreads();
                prefix_a();
                __syncthreads();
                wt = wtot[lane & (NW - 1)];
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
            if (i == QW - 1 && t == NT - 1) H[NB / 2] = base;         // base past the last bucket = number of non-NaN keys
        }
        __syncthreads();                                              // barrier 4
        // ---- (3) scatter (branch-free; NaNs write the dummy slot) ----
        b.lo = lo; b.hi = hi; b.scale = scale; b.flat = flat; b.trypure = trypure;
        b.nv = H[NB / 2];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const u32 bk = b.bs[e] & 0xFFFFu, slot = b.bs[e] >> 16;
            const u32 base = H16[bk];
            S[(bk < (u32)NB) ? base + slot : (u32)dummy] = k[e];
        }
        return b;
    }
};
#endif  // __HIPCC__

}  // namespace sd
