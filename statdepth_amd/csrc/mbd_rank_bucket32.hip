// mbd_rank_bucket32.hip -- K1+K2 bucket ranking on bucket-local key images, TWO workgroups per CU (J = 2, 3072 < n <= 11264).
//
// Same integers as rank_bucket_kernel (mbd_rank_bucket.hip), the pairwise kernel and the reference's enumeration
// (_functional.py:246-251, _containment.py:75-77).  The fp64 kernel keeps one row per CU in LDS and its five
// barrier-separated phases leave the VALU idle while the LDS works and the other way round (SQ counters: VALU busy 57 %,
// LDS busy 37 %, together the kernel's whole time).  Here a key is placed by a 31-bit image q(x), non-decreasing in x
// whatever the data and whatever the map's constants (round 4: a THREE-PIECE map -- a linear core of 14 336 buckets over the
// row's range, clipped to a central bracket of the bulk (taken from the threads' own minima and maxima) when the range is much wider than it
// (heavy tails, outlying curves), and below and above the core 1 024 buckets each for a float-like code of the distance to
// the core's edge, bits(d + c) - bits(c) with c = core width / 448: linear with the core's slope next to the edge, halving
// per octave, 32 octaves; every piece is monotone and the pieces are ordered): its top 14 bits are the key's bucket, and LDS
// holds a 31-bit BUCKET-LOCAL image -- q's low 17 bits followed by 14 more bits of the core's fraction, 45 bits of resolution in
// all (a tail key keeps q's 31: its 14 extra bits are 0; a core key's 45 bits are the mantissa of ONE fma, v = 2^38 + image,
// rounded to nearest: see convert4) -- so that a row of up to 11 264 curves + its 16 384-bucket
// histogram take 77 KiB and two 512-thread workgroups, half a row apart in phase, share a CU: one's compares run under the
// other's LDS traffic.  Order is decided by the images (within a bucket; buckets are ordered) wherever they differ; keys whose
// images coincide (two core values within range / 2^45, two tail values within the tail's 31-bit resolution, or equal values)
// are NOT ranked here: they are set aside with what the images do say (B0 = keys with a smaller image, E0 = keys with the same image)
// and settled exactly, in fp64, among themselves at the end of the workgroup (a group of equal images is complete in the list).
// Tie-heavy rows (quantised data: a bucket of 16 keys or more whose keys share an image) are ranked in closed form when
// every bucket of the row provably holds one value.
// The histogram's words: word k counts buckets 2k and 2k + 1 in two 16-bit halves (phase 1: one atomic per key, whose return
// value is the key's slot in its bucket; word and half are read off the two image words, r32_word_offset below).  The prefix
// sum turns word k of a row without a bucket of 64 keys into the PAIR WORD count(2k) | count(2k + 1) << 8 | base(2k) << 16
// and the scatter reads it ONCE per key, at the word address of the key's atomic
// (round 10; r32_pair_word, r32_pair_decode below); a crowded row's word keeps base(2k) | base(2k + 1) << 16 and its keys
// read the two halfwords b and b + 1 apart.  Word NB / 2 holds the number of non-NaN keys, word NB / 2 + 1 is the dummy counter
// of the NaN image.
// Rows this kernel does not take -- a NaN, an infinity, a bucket of 64 keys or more, ties mixed with near-ties, and
// every row of a workgroup whose list of set-aside keys overflows -- are flagged and ranked by rank_bucket_kernel's
// SEL form in a second launch that returns at once when nothing was flagged (gate word = the call's epoch).
//
// Per-curve totals stay in registers (u32: the host checked that a workgroup's total fits); one partial block per
// workgroup goes to HBM, stored non-temporally, and the second launch (rank_bucket_kernel's SEL form) sums the blocks into the
// totals.  HBM traffic: the matrix once + the partial blocks.
#include <atomic>

#include "sd_common.h"
#include "rank_routes.h"
#include "rank_bucket.h"

namespace sd {

constexpr int R32_PRIO_LDS = 2;                 // s_setprio in the load / histogram / prefix / scatter phases (issue on arrival)
constexpr int R32_PRIO_VALU = 0;                // ... and in the member pass, which is bound by VALU issue
constexpr int R32_MIN_N = 3072;                 // the two-launch path is used above this n (measured: -10 % at 4 096, nothing at 3 072)
constexpr int R32_LNB = 14;                     // 16 384 buckets: histogram 32 KiB
constexpr int R32_NT = 512, R32_NW = 8;
constexpr int R32_LCAP = 64;                    // set-aside keys per workgroup before it hands all its rows over
constexpr int R32_PAD = 12;                     // sentinel images behind the keys (two quads past the last partial quad)
constexpr u32 R32_TB = 1024;                    // buckets of each tail
constexpr int R32_TSH = 30;                     // tail code = (bits(d + c) - bits(c)) >> 30: 2^22 codes = 32 buckets per octave
constexpr double R32_CDIV = 1.0 / 448.0;        // c = core width / 448: the first octave continues the core's slope (32 * 448 = 14 336)
constexpr double R32_BETA = 2.0;                // the central bracket is widened by this many spans on either side
constexpr double R32_VBASE = 274877906944.0;    // 2^38: v = 2^38 + u has one ulp = 2^-14 image, its mantissa is the 45-bit image
constexpr u32 R32_VBASE_HI = 0x42500000u;       // high word of 2^38
constexpr u32 R32_SENT = 0x7FFFFFFFu;           // sentinel image behind the keys (masked off by the member pass: any value would do)

// Round 10: the words a key carries and reads between its histogram atomic and the scatter.
//   key word   (a register of the key, from its bucket b):  8 * (b & 1) | byte offset of histogram word b >> 1, << 5 | slot << 24.
//              Its low five bits are all that v_bfe reads of an offset or a width: 0 for an even bucket, 8 for an odd one.
//   pair word  (histogram word k behind the prefix sum of a row without a bucket of 64 keys: both counts are below 64):
//              count(2k) | count(2k + 1) << 8 | base(2k) << 16.
// With v = the key word: count = bfe(pair, v, 8) and base = (pair >> 16) + bfe(pair, 0, v), a field of no width for an even
// bucket and count(2k) for an odd one -- no select and no compare for the parity.
// Round 11: the key word is made from the two IMAGE words (vh = the high word of 2^38 + image, q = the low one), the bucket
// b = bits 31 .. 44 of the image is never put together.  Its histogram word b >> 1 is the low 14 bits of vh (13 bucket bits and
// the one that lets the NaN image reach word NB / 2 + 1), its parity is bit 31 of q: off4 = the word's byte offset -- the
// atomic's address and the field at bits 5 .. 20 -- and par = the parity give the word of bucket b = 2 * (off4 / 4) + par.
__device__ __forceinline__ u32 r32_word_offset(u32 vh) { return (vh << 2) & 0xFFFCu; }
__device__ __forceinline__ u32 r32_key_word(u32 off4, u32 par) { return (off4 << 5) | (par << 3); }
__device__ __forceinline__ u32 r32_key_word_offset(u32 kw) { return __builtin_amdgcn_ubfe(kw, 5u, 16u); }
__device__ __forceinline__ u32 r32_key_word_bucket(u32 kw) { return (__builtin_amdgcn_ubfe(kw, 7u, 14u) << 1) | ((kw >> 3) & 1u); }
// h = the word's two 16-bit counters: bytes 0 and 2 of h under bytes 0 and 1 of base, one v_perm_b32
__device__ __forceinline__ u32 r32_pair_word(u32 base, u32 h) { return __builtin_amdgcn_perm(base, h, 0x05040200u); }
__device__ __forceinline__ void r32_pair_decode(u32 pw, u32 kw, u32 &base, u32 &cnt) {
    cnt = __builtin_amdgcn_ubfe(pw, kw, 8u);
    base = (pw >> 16) + __builtin_amdgcn_ubfe(pw, 0u, kw);
}

template <int E, int LNB>
struct R32Cfg {
    static constexpr int NT = R32_NT, NW = R32_NW, NB = 1 << LNB;
    static constexpr int QW = NB / 2 / NT / 4;                  // 16-byte quads of histogram words per thread
    static_assert(QW >= 1 && NB / 2 == QW * 4 * NT, "whole quads of histogram words per thread");
    static constexpr int SH = 31 - LNB;
    static constexpr u32 C0 = R32_TB << SH, C1 = ((u32)NB - R32_TB) << SH;   // images of the core: [C0, C1)
    static constexpr u32 CU0 = 2u << SH, CU1 = ((u32)NB - 2u) << SH;         // ... of a row that is not clipped: [CU0, CU1)
    static_assert(C0 % (2u << SH) == 0 && C1 % (2u << SH) == 0 && CU0 % (2u << SH) == 0 && CU1 % (2u << SH) == 0,
                  "the core's bounds are whole steps of the high word of 2^38 + image (2^18 images)");
    static constexpr u32 NANIMG = ((u32)NB + 2u) << SH;         // a NaN's image: its bucket is the dummy counter NB + 2
    static_assert(LNB == 14, "the first tail octave continues the core's slope for 14 336 core buckets");
    static constexpr size_t HDR = 8 * NW * 8 + NW * 4 + 32 + (size_t)R32_LCAP * 8;
    static_assert(HDR % 16 == 0, "the histogram starts on a 16-byte boundary");
    static __host__ __device__ constexpr int al4(int n) { return (n + 3) & ~3; }
    static __host__ __device__ constexpr int pstride(int n) { return (n + 31) & ~31; }   // partial blocks: whole 128-byte lines
    static __host__ __device__ constexpr int dummy_pos(int n) { return al4(n) + R32_PAD; }
    static __host__ __device__ constexpr size_t lds_bytes(int n) { return HDR + (size_t)(NB / 2 + 4) * 4 + (size_t)(dummy_pos(n) + 4) * 4; }
};

template <int E, int LNB>
__global__ __launch_bounds__(R32_NT, 4) void rank_bucket32_kernel(const double *__restrict__ Y, i64 n64, i64 row0, i64 rows,
                                                                 u32 *__restrict__ partial, unsigned char *__restrict__ rowflag,
                                                                 u32 *__restrict__ gate, u32 epoch, u64 *__restrict__ out_zero) {
    using C = R32Cfg<E, LNB>;
    constexpr int NT = C::NT, NW = C::NW, NB = C::NB, QW = C::QW, SH = C::SH;
    constexpr u32 C0 = C::C0, C1 = C::C1, CU0 = C::CU0, CU1 = C::CU1, NANIMG = C::NANIMG;
    // A static block sized for the class's largest n (E * NT curves): every LDS address is a compile-time offset plus an
    // index, not the run-time base of a dynamic segment added to each of them.  The layout is the one lds_bytes(n) describes;
    // the run-time n only decides where the sentinels and the dummy lie inside it.
    constexpr size_t LDS = C::lds_bytes(E * NT);
    static_assert(2 * LDS <= 160 * 1024, "two workgroups per CU");
    // The member pass reads the quad behind the one a bucket starts in whether the bucket reaches it or not.  A base is at
    // most n - 1: its quad ends at word al4(n) - 1 and the next one at word al4(n) + 3, inside the dummy_pos(n) + 4 =
    // al4(n) + R32_PAD + 4 words of S for every n of the class, the largest included (the static block).
    static_assert(R32_PAD >= 0 && C::al4(E * NT) + 3 < C::dummy_pos(E * NT) + 4, "the second quad of the last bucket lies in S");
    __shared__ __attribute__((aligned(16))) double Sm[(LDS + 7) / 8];
    const int n = (int)n64;
    double *red = Sm;                                                 // [2][NW][4] min / max of the row, central bracket of its keys
    u32 *wtot = reinterpret_cast<u32 *>(red + 8 * NW);                // [NW]
    u32 *misc = wtot + NW;                                            // [0]: set-aside keys so far, [1]: running sum of the ranks
    u32 *lkey = misc + 8, *lbe = lkey + R32_LCAP;                     // (row index << 14 | curve), B0 | E0 << 16
    u32 *H = reinterpret_cast<u32 *>(reinterpret_cast<char *>(Sm) + C::HDR);
    u32 *S = H + NB / 2 + 4;                                          // key images in bucket order + sentinels + dummy
    const unsigned short *H16 = reinterpret_cast<const unsigned short *>(H);
    const int t0 = threadIdx.x;
    const double INF = __builtin_huge_val();
    const double QNAN = __builtin_nan("");
    const int DUMMY = C::dummy_pos(n);
    const u32 nm1 = (u32)n - 1u;
    const u32 ranksum = (u32)(((u64)n * (u64)(n - 1)) >> 1);          // sum of the ranks of a row without equal images
    int t = t0;

    if (blockIdx.x == 0 && t == 0) gate[2] = 0;                       // the second launch's arrival counter
    if (out_zero)                                                     // the second launch adds every total to out
        for (i64 c = (i64)blockIdx.x * NT + t; c < n; c += (i64)gridDim.x * NT) out_zero[c] = 0;
    for (int p = n + t; p < DUMMY + 4; p += NT) S[p] = R32_SENT;
    {
        uint4 *Hq = reinterpret_cast<uint4 *>(H);
#pragma unroll
        for (int i = 0; i < QW; ++i) Hq[i * NT + t] = make_uint4(0, 0, 0, 0);
        if (t < 4) H[NB / 2 + t] = 0;
        if (t < 5) misc[t] = 0;
    }

    // curves of thread t: t, t + NT, ...; slots beyond n read as NaN (they count into the dummy word like any NaN)
    double x[E];
    auto load_row = [&](i64 r) {
        const double *rp = Y + (row0 + r) * n + t;
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = (e < E - 2 || t + e * NT < n) ? rp[e * NT] : QNAN;   // n > (E - 2) * NT
    };
    u32 acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0;
    auto row_range = [&](int parity) {
        double mn = INF, mx = -INF;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            mn = rb_mm<false>(mn, x[e]);
            mx = rb_mm<true>(mx, x[e]);
        }
        // the central bracket (it only places the core: the map is monotone whatever it says), from the keys in hand: a thread's
        // keys are a strided subset of the row, so the minima and maxima of groups of 16 keys or more (one lane from E = 16 on,
        // 2 or 4 lanes below) are 32 small samples from all over the curve index, and the innermost of them -- the largest
        // minimum, the smallest maximum -- bracket the bulk.  In float; a group without a value is neutral.
        float2 wb = rb3_wave_bracket<E, NT>(mn, mx);
        // Two unrelated keys equal (curves 512 apart, up to ten pairs per thread: 3 584 pairs of a row or more, as many as the
        // round-4 sample compared; values 0.1 apart over a range of 200 escape 5 120 pairs in 3 rows of 1 000): values on a
        // grid.  Such a row is ranked in closed form when every bucket holds ONE value, which the tail buckets of a clipped
        // map -- octaves wide -- would spoil: an inverted bracket switches the clipping off for the row (its tails are no
        // heavier for being rounded; if they are heavy, the row is crowded and handed over as in round 3).  One clipped tie
        // row overflows the list and hands all its workgroup's rows over, so the test must not miss.
        {
            bool eqs = false;
#pragma unroll
            for (int e = 0; e < (E - 1 < 10 ? E - 1 : 10); ++e) eqs = eqs || (x[e] == x[e + 1]);   // (a slot beyond n is NaN: no)
            if (__ballot(eqs) != 0) {
                float finf = __builtin_huge_valf();
                asm volatile("" : "+v"(finf));                        // (set here: not a constant held in a register for the row loop)
                wb.x = finf;
                wb.y = -finf;
            }
        }
        const float imn = wb.x, imx = wb.y;
        mn = rb_wave_allreduce<false>(mn);
        mx = rb_wave_allreduce<true>(mx);
        double *rp = red + parity * 4 * NW;
        if ((t & 63) == 63) {
            double *wp = rp + 4 * (t >> 6);
            wp[0] = mn; wp[1] = mx;
            reinterpret_cast<float *>(wp + 2)[0] = imn;
            reinterpret_cast<float *>(wp + 2)[1] = imx;
        }
    };
    int par = 0;
    u32 rowidx = 0, nbad = 0, expect = 0;                             // block-uniform
    bool handover = false;                                            // the list overflowed: every row of this workgroup is handed over
    bool stop = false;
    u32 kb[E];                                                        // image, then B = keys with a smaller image (the rank)
    i64 r = blockIdx.x;
    for (; r < rows; r += gridDim.x) {
        t = t0;
        asm volatile("" : "+v"(t));                                   // addresses are recomputed per row, not hoisted and spilled
        const int lane = t & 63;
        const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
        // Tie-heavy / NaN-ridden data: when 8 of the first 16 workgroups have found their first row bad, everybody leaves what is left to
        // the second launch (gate[1] = epoch << 8 | count; block-uniform scalar load, a few rows stale at worst)
        if (rowidx && t == 0) misc[3] = __hip_atomic_load(gate + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ONE load per workgroup
        __builtin_amdgcn_s_setprio(R32_PRIO_LDS);                     // latency-bound phases go first, the compares of the member
        load_row(r);                                                  // pass (the other workgroup's, half a row away) fill in
        row_range(par);
        double *redp = red + par * 4 * NW;
        par ^= 1;
        __syncthreads();                                              // barrier 1 (histogram is zero, S is free)
        if (rowidx) {                                                 // block-uniform: everybody reads the word thread 0 fetched
            const u32 w = misc[3];
            if ((w >> 8) == (epoch & 0xFFFFFFu) && (w & 0xFFu) >= 8u) { stop = true; break; }
        }
        double lo, hi;                                                // the row's minimum and maximum, then the core of the map
        double mscale, moff, mc;
        u64 mcb;
        u32 mc0, mcw;                                                 // the core's first image and its width in images
        u32 mh0, mhw;                                                 // ... as high words of v = 2^38 + image: first, and how many
        bool go, bad;
        {
            const double2 p = reinterpret_cast<const double2 *>(redp)[2 * (lane & (NW - 1))];
            const float2 pb = reinterpret_cast<const float2 *>(redp + 4 * (lane & (NW - 1)) + 2)[0];
            lo = rb_readlane_f64(rb_row_allreduce<false>(p.x), 0);
            hi = rb_readlane_f64(rb_row_allreduce<true>(p.y), 0);
            const double imn = (double)__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(rb_row_allreduce_f32<true>(pb.x))));
            const double imx = (double)__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(rb_row_allreduce_f32<false>(pb.y))));
            // hi < lo: no value at this timepoint (every curve NaN), nothing is contained.  Else a row with an infinity, an
            // overflowing range or all values equal (one bucket) is handed over.
            const bool fin = (hi > lo) && (lo > -INF) && (hi < INF) && ((hi - lo) < INF);
            bad = !fin && (hi >= lo);
            // the core: the row's range, clipped to the central bracket widened by R32_BETA spans on either side (a
            // light-tailed row keeps its whole range and never sees the tail code; heavy tails and outlying curves go to the tails)
            const double si = imx - imn;
            u32 c0 = CU0, c1 = CU1;                                   // a light-tailed row: the core takes the whole image range
            if (fin && si > 0.0 && si < INF && (hi - lo) > (1.5 * (1.0 + 2.0 * R32_BETA)) * si) {   // block-uniform: the range is
                const double lo2 = imn - R32_BETA * si, hi2 = imx + R32_BETA * si;                  // much wider than the bulk
                lo = lo2 > lo ? lo2 : lo;
                hi = hi2 < hi ? hi2 : hi;
                c0 = C0;
                c1 = C1;
            }
            mc0 = c0;
            mcw = c1 - c0;
            const double wc = hi - lo;
            mscale = ((double)mcw - 64.0) / wc;                       // the largest key of an unclipped row stays inside the core
            moff = __builtin_fma(-lo, mscale, R32_VBASE + (double)c0);    // exact sum: lo lands on 2^38 + c0
            mh0 = R32_VBASE_HI + (c0 >> (SH + 1));
            mhw = mcw >> (SH + 1);
            mc = wc * R32_CDIV;
            mcb = (u64)__double_as_longlong(mc);
            go = fin && (wc > 0.0) && (mscale < INF) && (mc > 0.0);
            bad = bad || (fin && !go);
        }
        // images of four keys: a core key costs ONE fp64 instruction.  v = fma(x, mscale, moff) with moff = the core's offset + 2^38
        // lies in [2^38, 2^39) for a core key, where one ulp is 2^-14: the 52-bit mantissa of v IS the 45-bit image
        // I = round(2^14 u) (the fma's single rounding; u = the 31-bit image with its fraction), bucket = I >> 31 = bits 31 .. 44
        // of the two words, local image = the low word's 31 bits.  fma is monotone in x and the mantissa is monotone in v inside
        // the binade, so the image is non-decreasing in x whatever the constants.  The core's bounds are multiples of 2^18
        // images = one step of the high word: mh0 <= high word < mh0 + mhw is EXACTLY vlo <= v < vlo + mcw, and a NaN, a negative
        // v (sign bit: a huge unsigned word) or any other binade fails it.  The tail code is computed only when some lane of the
        // wave has a key outside the core; which side is read off v itself (monotone in x: v < vlo <=> below the core, also
        // for the row's minimum when the offset's rounding puts it a hair under the bound).  Out: the high image word in bk
        // (its low 14 bits: the bucket's histogram word), the low one in q -- the bucket-local image in its 31 bits (a tail
        // key: its 31-bit image's low 17 bits, 14 zero bits behind them) under the bucket's parity in bit 31, which STAYS there:
        // images are only ever compared inside one bucket (the member pass counts the bucket's own positions, the closed forms
        // read its first two slots), where it is the same bit for every key, and y - q has the sign of the 31-bit difference
        // with it as without it.  A slot that holds no
        // curve (!isk: its x is the NaN of load_row) is given the NaN's image directly and does not send its wave through the
        // tail code: at n = 10 000 half the waves of a workgroup have such a slot in every row.
        auto convert4 = [&](const double (&xv)[4], const bool (&isk)[4], u32 (&q)[4], u32 (&bk)[4]) {
            bool anyout = false;
            u32 vh[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const u64 w = (u64)__double_as_longlong(__builtin_fma(xv[i], mscale, moff));
                vh[i] = (u32)(w >> 32);
                q[i] = (u32)w;
                anyout = anyout || (isk[i] && vh[i] - mh0 >= mhw);
            }
            if (__ballot(anyout) != 0) {
                const double vlo = __longlong_as_double((long long)((u64)mh0 << 32));
                double zero = 0.0;
                asm volatile("" : "+v"(zero));                        // set here, where it is used: not a register pair held for the row loop
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool outc = vh[i] - mh0 >= mhw;
                    const bool low = __longlong_as_double((long long)(((u64)vh[i] << 32) | q[i])) < vlo;
                    double d = low ? lo - xv[i] : xv[i] - hi;
                    d = rb_mm<true>(d, zero);                         // a key the rounding put just outside: code 0
                    const u64 tc = ((u64)__double_as_longlong(d + mc) - mcb) >> R32_TSH;
                    // below the core: mc0 - 1 downwards; above: from the core's end upwards; clamped to what is left of the
                    // image range (a clipped core leaves 1 024 buckets on either side, an unclipped one two buckets: only a
                    // key the rounding put just outside comes here then)
                    const u32 room = low ? mc0 - 1u : 0x7FFFFEFFu - (mc0 + mcw);
                    const u32 tcc = tc < (u64)room ? (u32)tc : room;
                    u32 qt = low ? (mc0 - 1u) - tcc : (mc0 + mcw) + tcc;
                    qt = (xv[i] == xv[i]) ? qt : NANIMG;
                    vh[i] = outc ? qt >> (SH + 1) : vh[i];            // the words of qt << 14: a tail key keeps the 31-bit resolution
                    q[i] = outc ? qt << (31 - SH) : q[i];
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                vh[i] = isk[i] ? vh[i] : NANIMG >> (SH + 1);          // the words of NANIMG << 14, as the tail code gives a NaN
                q[i] = isk[i] ? q[i] : NANIMG << (31 - SH);
                bk[i] = vh[i];                                        // a NaN's image: the dummy counter NB + 2 (word NB / 2 + 1)
            }
        };
        u32 bc[E];                                                    // high image word, r32_key_word | slot << 24, then (at the scatter) base | count << 14
        if (go) {
            // ---- (1) image, bucket, slot ----

            // batches of 8 atomics in flight; their return values (the slots) are packed 4 to a register per batch
#pragma unroll
            for (int e0 = 0; e0 < E; e0 += 8) {
                u32 old[8];
#pragma unroll
                for (int h = 0; h < 8; h += 4) {
                    if (e0 + h < E) {
                        double xv[4];
                        u32 q[4], bk[4];
                        bool isk[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int e = e0 + h + i < E ? e0 + h + i : e0 + h;
                            xv[i] = x[e];
                            isk[i] = e < E - 2 || t + e * NT < n;
                        }
                        convert4(xv, isk, q, bk);
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (e0 + h + i < E) { kb[e0 + h + i] = q[i]; bc[e0 + h + i] = bk[i]; }
                    }
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int e = e0 + i;
                    if (e < E) {
                        // six vector instructions in front of the atomic (they are issued at the LDS phases' priority, where
                        // one costs about three times what it costs in the member pass: DESIGN S3, round 11)
                        const u32 off4 = r32_word_offset(bc[e]);
                        u32 par = kb[e] >> 31, one;
                        // 1 << 16 * parity = 0xFFFF * parity + 1: one v_mad_u32_u24 (written out: the compiler makes it a compare
                        // and a select, 20 cycles of issue), not two shifts
                        asm("v_mad_u32_u24 %0, %1, %2, 1" : "=v"(one) : "v"(par), "s"(0xFFFFu));
                        asm("" : "+v"(par));                          // (the key word from par, not from q again)
                        old[i] = atomicAdd(reinterpret_cast<u32 *>(reinterpret_cast<char *>(H) + off4), one);
                        bc[e] = r32_key_word(off4, par);
                    }
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int e = e0 + i;
                    if (e < E)   // (v_bfe reads five bits of its offset: 16 * parity.)  A NaN key's slot is read from the wrong
                        bc[e] |= __builtin_amdgcn_ubfe(old[i], bc[e] << 1, 8u) << 24;   // half: its row is not taken anyway
                }
#pragma unroll
                for (int i = 0; i < 8; ++i)                           // packed HERE: not (old, shift) pairs kept for the scatter
                    if (e0 + i < E) asm volatile("" : "+v"(bc[e0 + i]));
            }
            __syncthreads();                                          // barrier 2
            // ---- (2) exclusive prefix sum over the counters (conflict-free 16-byte accesses: lane <-> quad) ----
            uint4 *Hq = reinterpret_cast<uint4 *>(H) + wave * (64 * QW);
            uint4 hq[QW];
            u32 runq[QW], inclq[QW], offq[QW], ov = 0, wsum = 0;
#pragma unroll
            for (int i = 0; i < QW; ++i) {
                hq[i] = Hq[i * 64 + lane];
                const u32 s4 = hq[i].x + hq[i].y + hq[i].z + hq[i].w;
                ov |= hq[i].x | hq[i].y | hq[i].z | hq[i].w;          // bit k of a half set <=> some counter has it
                runq[i] = (s4 & 0xFFFFu) + (s4 >> 16);
                inclq[i] = rb_wave_incl_scan(runq[i]);
                offq[i] = wsum;
                wsum += rb_readlane(inclq[i], 63);
            }
            const bool wover = __ballot((ov & 0xFFC0FFC0u) != 0) != 0;   // some bucket holds 64 keys or more
            const bool wtry = __ballot((ov & 0xFFF0FFF0u) != 0) != 0;    // ... 16 or more: ties rather than density?
            if (lane == 63) wtot[wave] = wsum | (wover ? 0x80000000u : 0u) | (wtry ? 0x40000000u : 0u);
            __syncthreads();                                          // barrier 3
            const u32 wt = wtot[lane & (NW - 1)];
            const bool crowded = __ballot((wt >> 31) != 0) != 0;
            const bool trypure = __ballot((wt & 0x40000000u) != 0) != 0;
            const u32 wscan = rb_row_incl_scan(wt & 0x3FFFFFFFu);
            const u32 woff = wave ? rb_readlane(wscan, wave - 1) : 0u;
            // block-uniform.  No bucket of 64 keys: word k becomes the PAIR WORD of buckets 2k and 2k + 1 (r32_pair_word: both
            // counts and the even bucket's base), one 4-byte read per key at the scatter.  A crowded row's counts do not fit
            // it: that row keeps the two bases as halfwords and the two-read scatter.
#pragma unroll
            for (int i = 0; i < QW; ++i) {
                const u32 b0 = woff + offq[i] + inclq[i] - runq[i];
                const u32 b1 = b0 + (hq[i].x & 0xFFFFu) + (hq[i].x >> 16);
                const u32 b2 = b1 + (hq[i].y & 0xFFFFu) + (hq[i].y >> 16);
                const u32 b3 = b2 + (hq[i].z & 0xFFFFu) + (hq[i].z >> 16);
                uint4 o;
                if (!crowded) {
                    o.x = r32_pair_word(b0, hq[i].x);
                    o.y = r32_pair_word(b1, hq[i].y);
                    o.z = r32_pair_word(b2, hq[i].z);
                    o.w = r32_pair_word(b3, hq[i].w);
                } else {
                    o.x = b0 | ((b0 + (hq[i].x & 0xFFFFu)) << 16);
                    o.y = b1 | ((b1 + (hq[i].y & 0xFFFFu)) << 16);
                    o.z = b2 | ((b2 + (hq[i].z & 0xFFFFu)) << 16);
                    o.w = b3 | ((b3 + (hq[i].w & 0xFFFFu)) << 16);
                }
                Hq[i * 64 + lane] = o;
                if (i == QW - 1 && t == NT - 1)                       // base past the last bucket = number of non-NaN keys
                    H[NB / 2] = b3 + (hq[i].w & 0xFFFFu) + (hq[i].w >> 16);
            }
            __syncthreads();                                          // barrier 4
            const u32 nv = H[NB / 2];
            // block-uniform.  A crowded row (a bucket of 64 keys or more) is scattered too: its slots wrap at 256 but stay inside
            // their buckets, which is all the closed form below asks of S; its member pass is never run.
            bool take = nv == (u32)n;
            if (take && !crowded) {
                // ---- (3) scatter into bucket order: ONE 4-byte read per key, of the pair word its histogram atomic went to.
                //      One key at a time, read - decode - write: measured faster than batches of 2, 4, 5, 8 or 10 reads in
                //      flight, in that order (DESIGN S3, round 10) ----
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const u32 pw = *reinterpret_cast<const u32 *>(reinterpret_cast<const char *>(H) + r32_key_word_offset(bc[e]));
                    __builtin_amdgcn_sched_barrier(0);                // the next key's read is not moved up to this one
                    u32 base, cnt;
                    r32_pair_decode(pw, bc[e], base, cnt);
                    const bool isk = e < E - 2 || t + e * NT < n;
                    // (byte offsets: the slot sits two bits above the top byte's foot, so that kw >> 22 is 4 * slot)
                    *reinterpret_cast<u32 *>(reinterpret_cast<char *>(S) + (isk ? (base << 2) + (bc[e] >> 22) : (u32)DUMMY * 4u)) = kb[e];
                    // a slot beyond n carries the NaN image: its "bucket" is the dummy counter, not a range of S -- one key at 0
                    bc[e] = isk ? base | (cnt << 14) : (1u << 14);
                }
            } else if (take) {
                // ---- (3') a crowded row: the two bases of word k as halfwords (its member pass is never run) ----
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const u32 b = r32_key_word_bucket(bc[e]), slot = bc[e] >> 24;
                    // two 2-byte reads, kept apart: merged into one 4-byte read they sit on an odd halfword for every
                    // odd b, and the LDS replays such a read for 64 cycles (SQ_LDS_UNALIGNED_STALL)
                    u32 b1 = b + 1u;
                    asm("" : "+v"(b1));                               // adjacency hidden from the load vectoriser
                    const u32 base = H16[b], end = H16[b1];
                    const bool isk = e < E - 2 || t + e * NT < n;
                    S[isk ? base + slot : (u32)DUMMY] = kb[e];
                    // a slot beyond n carries the NaN image: its "bucket" is the dummy counter, not a range of S -- one key at 0
                    bc[e] = isk ? base | ((end - base) << 14) : (1u << 14);
                }
            }
            __syncthreads();                                          // barrier 5
            bool pure = false;                                        // block-uniform: the row is ranked in closed form
            if (take && (trypure || crowded)) {
                // A bucket of 16 keys or more is tie-heavy (quantised) data more often than a dense cluster.  When a key
                // there shares its image with the first two keys of its bucket, the row is tried in closed form: if every
                // bucket of the row holds ONE value, the ranks are B = base, A = n - base - count and there is no member
                // pass at all.  One value per bucket is PROVEN on the doubles: equal images (the first key's, in S), then
                // equal high and low words -- every key of a bucket writes its words to the bucket's first two slots (one
                // key's land) and all compare with what landed.  A row that fails any of it is handed over.
                const u32 tag = rowidx + 1u;                          // misc words tagged by the row: nothing to reset
                bool vote = false, same = true;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const u32 base = bc[e] & 0x3FFFu, cnt = bc[e] >> 14;
                    if (e < E - 2 || t + e * NT < n) {
                        const u32 first = S[base];
                        same = same && (first == kb[e]);
                        if (cnt >= 16u) vote = vote || (first == kb[e] && S[base + 1] == kb[e]);
                    }
                }
                if (vote) misc[2] = tag;
                if (!same) misc[4] = tag;
                __syncthreads();
                // tie-heavy: closed form, or hand-over when a bucket is beyond the member pass (64 keys); a row with a bucket of 16
                // equal keys whose other buckets mix values (a clipped map's tail buckets are octaves wide) takes the member pass
                if ((misc[2] == tag && misc[4] != tag) || crowded) {
                    take = false;
                    bool ok = misc[2] == tag && misc[4] != tag;       // block-uniform
                    if (ok) {
                        // the doubles again (L2; their registers went to the images); -0 counts as +0.  A bucket of two keys
                        // or more takes the high word in its first slot and the low word in its second.  Four keys at a time
                        // (loaded again for the comparison): this cold path must not cost the row loop its registers.
                        const double *rp = Y + (row0 + r) * n + t;
#pragma unroll
                        for (int pass = 0; pass < 2; ++pass) {
                            bool eq = true;
#pragma unroll
                            for (int e0 = 0; e0 < E; e0 += 4) {
                                int eo = e0 * NT;                     // opaque: one address computation per group, none hoisted
                                asm volatile("" : "+v"(eo));
                                const double *rq = rp + eo;
                                u64 w[4];
#pragma unroll
                                for (int i = 0; i < 4; ++i) {
                                    const bool isk = e0 + i < E && (e0 + i < E - 2 || t + (e0 + i) * NT < n);
                                    w[i] = (u64)__double_as_longlong((isk ? rq[i * NT] : 0.0) + 0.0);
                                }
#pragma unroll
                                for (int i = 0; i < 4; ++i) {
                                    if (e0 + i < E && (e0 + i < E - 2 || t + (e0 + i) * NT < n) && (bc[e0 + i] >> 14) >= 2u) {
                                        u32 *sp = S + (bc[e0 + i] & 0x3FFFu);
                                        if (pass == 0) { sp[0] = (u32)(w[i] >> 32); sp[1] = (u32)w[i]; }
                                        else eq = eq && sp[0] == (u32)(w[i] >> 32) && sp[1] == (u32)w[i];
                                    }
                                }
                                __builtin_amdgcn_sched_barrier(0);
                            }
                            if (pass == 1 && !eq) misc[4] = tag;
                            __syncthreads();
                        }
                        ok = misc[4] != tag;
                    }
                    if (ok) {
                        pure = true;
#pragma unroll
                        for (int e = 0; e < E; ++e) {
                            const u32 B = bc[e] & 0x3FFFu, A = (u32)n - B - (bc[e] >> 14);
                            acc[e] += (e < E - 2 || t + e * NT < n) ? (nm1 * (nm1 - 1u) - A * (A - 1u) - B * (B - 1u)) >> 1 : 0u;
                        }
                    }
                }
            }
            __builtin_amdgcn_s_setprio(R32_PRIO_VALU);
            {                                                         // the histogram is dead until the next row's atomics
                uint4 *Hz = reinterpret_cast<uint4 *>(H) + wave * (64 * QW);
#pragma unroll
                for (int i = 0; i < QW; ++i) Hz[i * 64 + lane] = make_uint4(0, 0, 0, 0);
                if (t < 2) H[NB / 2 + t] = 0;
            }
            if (take) {
                // ---- (4) rank inside the bucket: two quads from the 16-byte boundary at or below the bucket's base.  Images
                //      are bucket-local, so only the bucket's own positions [off, off + cnt) of the window are counted (the
                //      keys of other buckets around them are masked off; the second quad is read where it lies, through the
                //      first one's address register, whether the bucket reaches it or not: the next buckets' keys, the
                //      sentinels or the padding behind them).  Only `<` is counted: equal images show in the sum of the row's ranks
                //      (fold below) ----
                const uint4 *S4 = reinterpret_cast<const uint4 *>(S);
                uint4 y0, y1;
                auto window = [&](int e) {
                    const u32 base = bc[e] & 0x3FFFu;
                    const uint4 *p = S4 + (base >> 2);
                    y0 = p[0];
                    y1 = p[1];                                        // whether the bucket reaches it or not (the static_assert above)
                };
                u32 sB = 0;
                window(0);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const u32 base = bc[e] & 0x3FFFu, cnt = bc[e] >> 14, off = base & 3u;
                    const u32 qe = kb[e];
                    // y < q <=> bit 31 of y - q (images below 2^31 under one parity bit); v_alignbit shifts it into a bit list (window position p
                    // at bit p): two full-rate instructions per member and no compare -> carry chain through vcc (gfx950
                    // pays wait states on those)
                    u32 lt = 0;
                    lt = __builtin_amdgcn_alignbit(lt, y1.w - qe, 31);
                    lt = __builtin_amdgcn_alignbit(lt, y1.z - qe, 31);
                    lt = __builtin_amdgcn_alignbit(lt, y1.y - qe, 31);
                    lt = __builtin_amdgcn_alignbit(lt, y1.x - qe, 31);
                    lt = __builtin_amdgcn_alignbit(lt, y0.w - qe, 31);
                    lt = __builtin_amdgcn_alignbit(lt, y0.z - qe, 31);
                    lt = __builtin_amdgcn_alignbit(lt, y0.y - qe, 31);
                    lt = __builtin_amdgcn_alignbit(lt, y0.x - qe, 31);
                    if (e + 1 < E) window(e + 1);
                    u32 less = (u32)__popc(__builtin_amdgcn_ubfe(lt, off, cnt < 8u ? cnt : 8u));   // the members only
                    if (cnt + off > 8u) {                             // the rest of a long bucket (a few lanes per visit)
                        const uint4 *p = S4 + (base >> 2);
#pragma unroll 1
                        for (u32 kk = 8; kk < cnt + off; kk += 4) {   // up to 63 + 3 positions: the bit list is counted per quad
                            const uint4 y = p[kk >> 2];
                            const u32 rest = cnt + off - kk;          // members left: the last quad may run into the next bucket
                            u32 l4 = 0;
                            l4 = __builtin_amdgcn_alignbit(l4, y.w - qe, 31);
                            l4 = __builtin_amdgcn_alignbit(l4, y.z - qe, 31);
                            l4 = __builtin_amdgcn_alignbit(l4, y.y - qe, 31);
                            l4 = __builtin_amdgcn_alignbit(l4, y.x - qe, 31);
                            less += (u32)__popc(__builtin_amdgcn_ubfe(l4, 0u, rest < 4u ? rest : 4u));
                        }
                    }
                    const u32 B = base + less;                        // keys with a smaller image
                    kb[e] = B;
                    const bool isk = e < E - 2 || t + e * NT < n;
                    sB += isk ? B : 0u;
                    acc[e] += isk ? __umul24(B, nm1 - B) : 0u;        // contained pairs = A * B, taken back below if B is not the rank
                    __builtin_amdgcn_sched_barrier(0);                // one window ahead, not more: the registers are counted
                }
                sB = rb_wave_incl_scan(sB);
                if (lane == 63) atomicAdd(&misc[1], sB);
                __syncthreads();                                      // barrier 6: the row's rank sum is complete
                {
                    // ---- fold of the row.  Its ranks are exact iff no two images coincide, i.e. iff they are a
                    //      permutation of 0 .. n-1, i.e. iff they sum to n(n-1)/2 (equal images share the smaller rank) ----
                    const u32 have_sum = misc[1];
                    expect += ranksum;
                    if (have_sum != expect) {
                        // Keys with equal images have equal B: counted through the (empty) histogram as u16 counters indexed by
                        // B.  The tied ones take their product back and are set aside with B0 = B and the size of their group.
                        expect = have_sum;
                        const u32 l0 = misc[0];                       // the list before this row (no push since the last barrier)
#pragma unroll
                        for (int e = 0; e < E; ++e)
                            if (e < E - 2 || t + e * NT < n) atomicAdd(&H[kb[e] >> 1], 1u << ((kb[e] & 1u) * 16u));
                        __syncthreads();
#pragma unroll
                        for (int e = 0; e < E; ++e) {
                            if (e < E - 2 || t + e * NT < n) {
                                const u32 B = kb[e], c = H16[B];
                                if (c != 1u) {
                                    acc[e] -= __umul24(B, nm1 - B);
                                    const u32 idx = atomicAdd(&misc[0], 1u);
                                    if (idx < (u32)R32_LCAP) {
                                        lkey[idx] = (rowidx << 14) | (u32)(t + e * NT);
                                        lbe[idx] = B | (c << 16);
                                    }
                                }
                            }
                        }
                        __syncthreads();
                        // (E <= 16, n <= 8 192: from E = 18 on this cold code costs the row loop two accumulators in scratch,
                        // + 5 % on config 2; there a bucket of 16 equal keys is common on such data and the closed form above runs)
                        if (E <= 16 && misc[0] > (u32)R32_LCAP) {     // block-uniform
                            // More tied keys than the list takes: values on a grid (rounded measurements) with a few equal keys
                            // per bucket -- too few for the closed form above to be tried.  Keys with equal images share B, the
                            // group of B occupies the sorted positions B .. B + c - 1, so its first two slots of S (dead: the
                            // member pass is over) take the words of its doubles as above: if every group holds ONE value, a tied
                            // key has B curves strictly below and n - B - c strictly above, and the list is not needed.
                            const u32 tag = (rowidx + 1u) | 0x40000000u;       // (not the closed form's tag above: it may have failed on this row)
                            const double *rp = Y + (row0 + r) * n + t;
#pragma unroll
                            for (int pass = 0; pass < 2; ++pass) {
                                bool eq = true;
#pragma unroll
                                for (int e0 = 0; e0 < E; e0 += 2) {
                                    int eo = e0 * NT;
                                    asm volatile("" : "+v"(eo));
                                    const double *rq = rp + eo;
                                    u64 w[2];
#pragma unroll
                                    for (int i = 0; i < 2; ++i) {
                                        const bool isk = e0 + i < E && (e0 + i < E - 2 || t + (e0 + i) * NT < n);
                                        w[i] = (u64)__double_as_longlong((isk ? rq[i * NT] : 0.0) + 0.0);
                                    }
#pragma unroll
                                    for (int i = 0; i < 2; ++i) {
                                        if (e0 + i < E && (e0 + i < E - 2 || t + (e0 + i) * NT < n) && H16[kb[e0 + i]] >= 2u) {
                                            u32 *sp = S + kb[e0 + i];
                                            if (pass == 0) { sp[0] = (u32)(w[i] >> 32); sp[1] = (u32)w[i]; }
                                            else eq = eq && sp[0] == (u32)(w[i] >> 32) && sp[1] == (u32)w[i];
                                        }
                                    }
                                    __builtin_amdgcn_sched_barrier(0);
                                }
                                if (pass == 1 && !eq) misc[4] = tag;
                                __syncthreads();
                            }
                            if (misc[4] != tag) {                     // block-uniform: proven
#pragma unroll
                                for (int e = 0; e < E; ++e) {
                                    if (e < E - 2 || t + e * NT < n) {
                                        const u32 B = kb[e], c = H16[B];
                                        if (c != 1u) {
                                            const u32 A = (u32)n - B - c;
                                            acc[e] += (nm1 * (nm1 - 1u) - A * (A - 1u) - B * (B - 1u)) >> 1;
                                        }
                                    }
                                }
                                if (t == 0) misc[0] = l0;             // this row's entries are dropped
                            }
                            __syncthreads();
                        }
#pragma unroll
                        for (int e = 0; e < E; ++e)
                            if (e < E - 2 || t + e * NT < n) H[kb[e] >> 1] = 0;
                        __syncthreads();
                        if (misc[0] > (u32)R32_LCAP) handover = true;     // block-uniform
                    }
                }
            } else {
                bad = !pure;
            }
        }
        if (t == 0) rowflag[r] = bad ? 1 : 0;
        nbad += bad ? 1u : 0u;
        ++rowidx;
        if (handover) break;
        if (bad && rowidx == 1 && t == 0 && blockIdx.x < 16) {        // my first row was bad: count me in (16 contenders at most)
            u32 old = gate[1], assumed;
            do {
                assumed = old;
                const u32 want = ((assumed >> 8) != (epoch & 0xFFFFFFu)) ? (((epoch & 0xFFFFFFu) << 8) | 1u)
                                 : ((assumed & 0xFFu) == 0xFFu ? assumed : assumed + 1u);
                old = atomicCAS(gate + 1, assumed, want);
            } while (old != assumed);
        }
        if (nbad >= 2 && 2 * nbad > rowidx) { stop = true; r += gridDim.x; break; }   // this data is not for this kernel: leave the rest
    }
    t = t0;
    __syncthreads();
    const u32 L = __builtin_amdgcn_readfirstlane(handover ? 0u : misc[0]);   // set-aside keys (an overflowing list hands over)
    if (handover) {                                                   // every row of this workgroup, ranked or not
        for (i64 rr = blockIdx.x + (i64)t * gridDim.x; rr < rows; rr += (i64)NT * gridDim.x) rowflag[rr] = 1;
        nbad = 1;
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = 0;
    } else if (stop) {
        for (i64 rr = r + (i64)t * gridDim.x; rr < rows; rr += (i64)NT * gridDim.x) rowflag[rr] = 1;   // rows left behind
    }
    // (stop with nbad == 0: gate[1] held this epoch's "eight contenders" before the launch -- stale workspace contents.  The rows
    // left behind are flagged above, so the gate opens for them as for any other flagged row.)
    if (t == 0 && (nbad || stop)) *gate = epoch;
    // ---- keys whose images coincide, settled among themselves in fp64 (their rows are NaN-free and finite, a group of equal
    //      images is complete in the list): wave 0, one listed key per lane, fetches the doubles (ONE round trip, issued ahead
    //      of the block's stores), compares within the groups of equal (row, B0) through readlane and adds each key's
    //      closed-form term to its curve's entry of the block, behind the owners' stores ----
    u32 key = 0, be = 0;
    double xv = 0.0;
    if ((u32)t < L) {
        key = lkey[t];
        be = lbe[t];
        xv = Y[(row0 + (i64)blockIdx.x + (i64)(key >> 14) * gridDim.x) * n + (key & 0x3FFFu)];
    }
    // non-temporal: the blocks stream out as the workgroups end instead of sitting dirty in L2 at the kernel boundary
    u32 *P = partial + (size_t)blockIdx.x * C::pstride(n);           // blocks on 128-byte lines whatever n
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (e < E - 2 || t + e * NT < n) __builtin_nontemporal_store(acc[e], &P[t + e * NT]);
    if (L) {                                                          // block-uniform
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the owners' stores have reached L2 (the barrier alone
        __syncthreads();                                              // orders them only inside the CU) before the atomics
        if (t < 64) {                                                 // L <= R32_LCAP = 64: all of them in wave 0
            u32 B = be & 0xFFFFu, A = (u32)n - B - (be >> 16);
            for (u32 j = 0; j < L; ++j) {
                const u32 kj = rb_readlane(key, (int)j), bj = rb_readlane(be, (int)j);
                const double xj = rb_readlane_f64(xv, (int)j);
                if (j != (u32)t && (kj >> 14) == (key >> 14) && (bj & 0xFFFFu) == (be & 0xFFFFu)) {
                    B += (xj < xv) ? 1u : 0u;                         // -0 == +0: equal values count on neither side
                    A += (xj > xv) ? 1u : 0u;
                }
            }
            // the same curve may be listed in several rows; the term replaces the product the fold took back
            if ((u32)t < L) atomicAdd(&P[key & 0x3FFFu], (nm1 * (nm1 - 1u) - A * (A - 1u) - B * (B - 1u)) >> 1);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
bool rank_bucket32_supported(i64 n, i64 rows, int cus) {
    // u32 totals per workgroup, for this kernel's workgroups and for the fp64 kernel's when every row is handed over
    const u64 per = (u64)((rows + cus - 1) / cus) * (u64)n * (u64)n;
    return n > R32_MIN_N && n <= 11264 && rows >= cus && rows <= 4096 && per < ((u64)1 << 32) && xswitch("SD_RB_NO32") == 0;
}

size_t rank_bucket32_extra_bytes(i64 rows) { return align_up((size_t)rows + 64, 256); }

template <int E>
static int launch32_cfg(const double *Y, i64 n, i64 row0, i64 rows, u32 *partial, unsigned char *rowflag, u32 *gate, u32 epoch,
                        u64 *out_zero, int G, hipStream_t s) {
    auto kf = rank_bucket32_kernel<E, R32_LNB>;
    if (n > (i64)E * R32_NT || n <= (i64)(E - 2) * R32_NT)            // the kernel's static LDS block holds E * NT keys
        return fail(SD_ERR_UNSUPPORTED, "bucket32 kernel: n=%lld is not of the class E=%d", (long long)n, E);
    hipLaunchKernelGGL(kf, dim3(G), dim3(R32_NT), 0, s, Y, n, row0, rows, partial, rowflag, gate, epoch, out_zero);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

// rows [row0, row0 + rows): u32 partial totals of every curve per workgroup (G blocks of n), flags of the rows left to the
// fp64 kernel in rowflag[rows], *gate = epoch when there is any
int launch_rank_bucket32(const double *Y, i64 n, i64 row0, i64 rows, u32 *partial, unsigned char *rowflag, u32 *gate, u32 epoch,
                         u64 *out_zero, int G, hipStream_t s) {
    switch ((int)((n + 1023) / 1024)) {
        case 3: return launch32_cfg<6>(Y, n, row0, rows, partial, rowflag, gate, epoch, out_zero, G, s);
        case 4: return launch32_cfg<8>(Y, n, row0, rows, partial, rowflag, gate, epoch, out_zero, G, s);
        case 5: return launch32_cfg<10>(Y, n, row0, rows, partial, rowflag, gate, epoch, out_zero, G, s);
        case 6: return launch32_cfg<12>(Y, n, row0, rows, partial, rowflag, gate, epoch, out_zero, G, s);
        case 7: return launch32_cfg<14>(Y, n, row0, rows, partial, rowflag, gate, epoch, out_zero, G, s);
        case 8: return launch32_cfg<16>(Y, n, row0, rows, partial, rowflag, gate, epoch, out_zero, G, s);
        case 9: return launch32_cfg<18>(Y, n, row0, rows, partial, rowflag, gate, epoch, out_zero, G, s);
        case 10: return launch32_cfg<20>(Y, n, row0, rows, partial, rowflag, gate, epoch, out_zero, G, s);
        case 11: return launch32_cfg<22>(Y, n, row0, rows, partial, rowflag, gate, epoch, out_zero, G, s);
    }
    return fail(SD_ERR_UNSUPPORTED, "bucket32 kernel covers 3072 < n <= 11264");
}

u32 rank_bucket32_epoch() {
    static std::atomic<u32> counter{0};
    u32 e = ++counter;
    if (e == 0) e = ++counter;
    return e;
}

}  // namespace sd
