// bd_strict.hip -- K3: strict band depth (relax=False, the reference's default): the route plan, the workspace layout and
// the mask / matching pipeline.
// Replaces the subset loop of _univariate_band_depth (_functional.py:246-251) with `containment // len(curve)`
// (_containment.py:80): a j-subset of the other curves counts only if its band contains the target at EVERY timepoint.
//
// Per target, every curve i gets two T-bit masks over the timepoints:
//   UN_i[t] = (x_i > x_q) or x_i is NaN,   DN_i[t] = (x_i < x_q) or x_i is NaN.
// With pandas' skipna min/max (_containment.py:68-69) a subset fails at t iff all its members are in UN or all are in DN, so
// it is contained at every t iff AND_members(UN) == 0 and AND_members(DN) == 0 (as T-bit masks).  A NaN in the target fails
// everything (count 0).
//
// Which route a call takes is strict_plan's decision (StrictPlan, strict_routes.h, names them all).  This file has the general
// one, per batch of targets: masks (from a rank image where there is one) -> digests of the canonical masks -> pairs of CLEAN
// curves counted by grouping complementary masks -> pairs with a DIRTY curve (tie / NaN) tested, for the targets that have
// any; and the first generation behind it (T > 1024, J = 3, 4).  Short series: bd_strict_class.hip, bd_strict_grid.hip;
// explicit blocks: bd_strict_subsets.hip.
// Integer / compare work throughout: VALU-issue and LDS bound, no MFMA.
#include "sd_common.h"
#include "rank_routes.h"

namespace sd {

constexpr int ST_WREG = 16;          // first generation: mask words kept in registers (T <= 1024)

// masks[b][i][0..W) = UN, masks[b][i][W..2W) = DN
__global__ __launch_bounds__(ST_THREADS) void strict_masks_kernel(
    const double *__restrict__ Y, i64 T, i64 n, const i64 *__restrict__ targets, i64 q0,
    u64 *__restrict__ masks, u32 *__restrict__ xnan, const u32 *__restrict__ gate, const double *__restrict__ Yt) {
    i64 i = (i64)blockIdx.x * ST_THREADS + threadIdx.x;
    i64 b = blockIdx.y;
    if (gate && gate[b * 4] == 0) return;      // target already counted by complement matching
    i64 q = q0 + b;
    i64 tg = targets ? targets[q] : q;
    const double *tq = Yt ? Yt + b * (((T + 31) / 32) * 32) : nullptr;   // external targets: the gathered copy
    i64 W = (T + 63) / 64;
    u64 *mrow = masks + ((size_t)b * n + (i < n ? i : 0)) * 2 * W;
    bool anynan = false;
    for (i64 w = 0; w < W; ++w) {
        u64 un = 0, dn = 0;
        i64 tend = (w + 1) * 64 < T ? (w + 1) * 64 : T;
        for (i64 t = w * 64; t < tend; ++t) {
            double xq = tq ? tq[t] : Y[t * n + tg];
            double xi = i < n ? Y[t * n + i] : 0.0;
            anynan |= (xq != xq);
            u64 bit = (u64)1 << (t & 63);
            bool isn = xi != xi;
            if (xi > xq || isn) un |= bit;
            if (xi < xq || isn) dn |= bit;
        }
        if (i < n) {
            mrow[w] = un;
            mrow[W + w] = dn;
        }
    }
    if (anynan && blockIdx.x == 0 && threadIdx.x == 0) xnan[b] = 1;
}

template <typename Tv>
__device__ __forceinline__ Tv block_sum(Tv v, Tv *scratch) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    Tv r = 0;
    if (threadIdx.x == 0)
        for (unsigned k = 0; k < (blockDim.x + 63) / 64; ++k) r += scratch[k];
    return r;
}

// J = 2: pairs (a < b).  grid = (a tiles, b chunks, batch)
constexpr int ST_BCHUNK = 512;

template <bool REG>
__global__ __launch_bounds__(ST_THREADS) void strict_pairs_kernel(
    const u64 *__restrict__ masks, i64 T, i64 n, const i64 *__restrict__ targets, i64 q0,
    const u32 *__restrict__ xnan, const u32 *__restrict__ gate, u64 *__restrict__ out, int jcols) {
    __shared__ u64 scratch[ST_THREADS / 64];
    i64 b = blockIdx.z;
    i64 q = q0 + b;
    if (xnan[b]) return;                       // NaN in the target: nothing is contained
    if (gate && gate[b * 4] == 0) return;      // target already counted by complement matching
    i64 tg = targets ? targets[q] : q;
    i64 a = (i64)blockIdx.x * ST_THREADS + threadIdx.x;
    i64 b0 = (i64)blockIdx.y * ST_BCHUNK;
    i64 b1 = b0 + ST_BCHUNK < n ? b0 + ST_BCHUNK : n;
    i64 amin = (i64)blockIdx.x * ST_THREADS;
    if (b1 - 1 <= amin) return;                // whole chunk at or below the tile: no a < b pair
    int W = (int)((T + 63) / 64);
    const u64 *mb = masks + (size_t)b * n * 2 * W;
    bool alive = a < n && a != tg;
    const u64 *ma = mb + (size_t)(alive ? a : 0) * 2 * W;
    u64 un[ST_WREG], dn[ST_WREG];
    if constexpr (REG) {
#pragma unroll
        for (int w = 0; w < ST_WREG; ++w) {
            un[w] = (w < W) ? ma[w] : 0;
            dn[w] = (w < W) ? ma[W + w] : 0;
        }
    }
    u64 good = 0;
    for (i64 c = b0; c < b1; ++c) {
        if (c == tg) continue;
        const u64 *mc = mb + (size_t)c * 2 * W;   // wave-uniform: scalar loads
        // lanes that cannot count any more (dead lane, a >= c, or already in conflict with c) are "settled";
        // once the whole wave is settled the remaining words are skipped.  Most pairs conflict in the first
        // 64 timepoints, so this cuts the mask work by up to W (16 at T = 1000).
        u64 bad = (alive && a < c) ? 0 : ~0ull;
        if constexpr (REG) {
#pragma unroll
            for (int w = 0; w < ST_WREG; ++w) {
                if (w < W) {
                    bad |= (un[w] & mc[w]) | (dn[w] & mc[W + w]);
                    if ((w & 1) == 0 && __ballot(bad == 0) == 0) break;
                }
            }
        } else {
            for (int w = 0; w < W; ++w) {
                bad |= (ma[w] & mc[w]) | (ma[W + w] & mc[W + w]);
                if (__ballot(bad == 0) == 0) break;
            }
        }
        good += (bad == 0);
    }
    u64 tot = block_sum(good, scratch);
    if (threadIdx.x == 0 && tot) atomicAdd(&out[q * jcols], tot);
}

// ---------------------------------------------------------------------------------------------------
// J = 2, second generation (T <= 1024): 32-bit mask words in a word-major image m32[b][k][i] (k < W32: UN word k,
// k >= W32: DN word k - W32; the n curves of one word are contiguous, so every access below is coalesced).
//  strict_masks2_kernel  thread = curve, block = 256 curves x one word (32 timepoints) x a group of 32 targets: the
//      curve's 32 values stay in VGPRs across the targets (the first generation re-read the matrix once per target:
//      m n T loads from L2), the target's values are wave-uniform scalar loads.
//  strict_pairs2_kernel  the lane's own masks live in VGPRs (32 + 32 words); the partners come in sub-chunks of 64
//      whose masks are staged in LDS (16 KiB).  Pass 1 tests the first four words (128 timepoints) of every partner
//      branch-free (wave-uniform LDS addresses: broadcasts) and records the survivors as one bit per partner; pass 2
//      walks the remaining words only for the survivors (most pairs conflict early).  The first generation read the
//      partner's words through the scalar cache inside a loop with an early exit, which serialised on the
//      scalar-load latency (~1500 cycles per partner and wave).
// ---------------------------------------------------------------------------------------------------
constexpr int ST_W32 = 32;                  // mask words per kind kept in registers (T <= 1024)
constexpr int ST_TG = 32;                   // targets per block of the mask kernel
constexpr int ST_SUB = 64;

// How the mask kernels store a (target, curve, word) pair.  FULL: UN and DN words (the pair kernel's input).  With
// matching on, the first pass over a batch stores UN only and notes in dflag[b][i] whether the curve is dirty for the
// target (tie or NaN at a timepoint that counts: the only thing the matching needs DN for); DN words -- half of the
// largest traffic of the strict path -- are then written by a second pass over the targets that have dirty curves
// (dlist / *dcount, appended by the matching), which continuous data never runs.
struct StrictMaskOut {
    u32 *m32;
    unsigned char *dflag;      // null: FULL
    const u32 *cmask;          // with dflag: timepoints that do not count
    const u32 *tiemask;        // rank kernel: timepoints at which some two curves hold the same value (null: unknown)
    const u32 *dlist;          // null: every target of the batch, else the listed ones
    const u32 *dcount;
};
__device__ __forceinline__ void strict_store_masks(const StrictMaskOut &o, i64 b, int k, int W32, i64 n, i64 i, u32 un, u32 dn,
                                                   u32 valid) {
    if (i >= n) return;
    o.m32[((size_t)b * 2 * W32 + k) * n + i] = un;
    if (!o.dflag) {
        o.m32[((size_t)b * 2 * W32 + W32 + k) * n + i] = dn;
    } else {
        const u32 v = valid & ~o.cmask[k];
        if ((((un ^ dn) & v) != v) || (un & dn)) o.dflag[(size_t)b * n + i] = 1;      // rare: continuous data never stores
    }
}

// The batch's target curves, gathered curve-major and padded to whole words: Yt[b][t], t < Tp = 32 W32 (zero beyond T).
// The mask kernel then fetches a target's 32 values of a word with a few wide scalar loads instead of 32 strided ones;
// a NaN anywhere in the target is noted here.  grid = nb
__global__ __launch_bounds__(ST_THREADS) void strict_gather_targets_kernel(
    const double *__restrict__ Y, i64 T, i64 n, const i64 *__restrict__ targets, i64 q0, const double *__restrict__ Q,
    i64 mq, double *__restrict__ Yt, u32 *__restrict__ xnan) {
    const i64 b = blockIdx.x;
    const i64 tg = Q ? q0 + b : (targets ? targets[q0 + b] : q0 + b);      // Q: external targets, T x mq time-major
    const double *src = Q ? Q : Y;
    const i64 ld = Q ? mq : n;
    const i64 Tp = ((T + 31) / 32) * 32;
    bool isn = false;
    for (i64 t = threadIdx.x; t < Tp; t += ST_THREADS) {
        const double v = t < T ? src[t * ld + tg] : 0.0;
        isn |= v != v;
        Yt[b * Tp + t] = v;
    }
    if (__syncthreads_or(isn) && threadIdx.x == 0) xnan[b] = 1;
}

// grid = (ceil(n / 256), W32, ceil(nb / ST_TG))
__global__ __launch_bounds__(ST_THREADS) void strict_masks2_kernel(
    const double *__restrict__ Y, const double *__restrict__ Yt, i64 T, i64 n, i64 nb, StrictMaskOut o) {
    const i64 cnt = o.dlist ? (i64)*o.dcount : nb;
    const i64 z0 = (i64)blockIdx.z * ST_TG;
    if (z0 >= cnt) return;
    const i64 zend = z0 + ST_TG < cnt ? z0 + ST_TG : cnt;
    const i64 i = (i64)blockIdx.x * ST_THREADS + threadIdx.x;
    const int k = blockIdx.y;
    const int W32 = (int)((T + 31) / 32);
    const i64 t0 = (i64)k * 32;
    const int tl = (int)(T - t0 < 32 ? T - t0 : 32);
    const u32 valid = tl == 32 ? 0xFFFFFFFFu : ((1u << tl) - 1u);
    double x[32];
    u32 nanbits = 0;
#pragma unroll
    for (int t = 0; t < 32; ++t) {
        x[t] = (i < n && t < tl) ? Y[(t0 + t) * n + i] : 0.0;
        nanbits |= (x[t] != x[t]) ? (1u << t) : 0u;
    }
    for (i64 z = z0; z < zend; ++z) {
        const i64 b = o.dlist ? (i64)o.dlist[z] : z;
        const double *__restrict__ xq = Yt + (b * W32 + k) * 32;    // wave-uniform, contiguous: wide scalar loads
        u32 un = nanbits, dn = nanbits;
#pragma unroll
        for (int t = 0; t < 32; ++t) {                              // no branch in here: the loads issue together
            const double q = xq[t];
            un |= (x[t] > q) ? (1u << t) : 0u;
            dn |= (x[t] < q) ? (1u << t) : 0u;
        }
        strict_store_masks(o, b, k, W32, n, i, un & valid, dn & valid, valid);
    }
}

// The same masks from INTEGER ranks (n <= 32 767).  The bucket kernel's image mode (mbd_rank_bucket.hip) turns the
// matrix into R[t][i] = B | A << 16 with B = number of curves strictly below curve i at t (0xFFFFFFFF: NaN): B is order-
// and tie-preserving (x_i > x_q <=> B_i > B_q, equal values share B), costs one pass of the headline kernel (0.07 ms at
// 10 000 x 1 000), and makes the mask kernel's compares 32-bit (full rate; the fp64 ones run at half) on half the
// registers.  Rt: the batch's targets gathered as in strict_gather_targets_kernel (B only, zero beyond T).
constexpr u32 ST_RANK_NAN = 0xFFFFFFFFu;
// Which timepoints have two curves with the same value at all?  (A + B + 1 < number of non-NaN curves for some key of
// the row.)  Where none has, no curve can tie with any target and the mask kernel skips the tie test.  grid = T
__global__ __launch_bounds__(ST_THREADS) void strict_row_ties_kernel(const u32 *__restrict__ R, const u32 *__restrict__ rnan,
                                                                    i64 n, u32 *__restrict__ tiemask) {
    const i64 t = blockIdx.x;
    const u32 nv = (u32)n - rnan[t];
    bool tie = false;
    for (i64 i = threadIdx.x; i < n; i += ST_THREADS) {
        const u32 w = R[t * n + i];
        tie |= w != ST_RANK_NAN && (w >> 16) + (w & 0xFFFFu) + 1u != nv;
    }
    if (__syncthreads_or(tie) && threadIdx.x == 0) atomicOr(&tiemask[t >> 5], 1u << (t & 31));
}

__global__ __launch_bounds__(ST_THREADS) void strict_gather_rank_targets_kernel(
    const u32 *__restrict__ R, i64 T, i64 n, const i64 *__restrict__ targets, i64 q0, u32 *__restrict__ Rt,
    u32 *__restrict__ xnan) {
    const i64 b = blockIdx.x;
    const i64 tg = targets ? targets[q0 + b] : q0 + b;
    const i64 Tp = ((T + 31) / 32) * 32;
    bool isn = false;
    // packed for the mask kernel: word k's timepoints j and j + 16 share Rt[b][16 k + j] (low / high half)
    for (i64 e = threadIdx.x; e < Tp / 2; e += ST_THREADS) {
        const i64 t = (e / 16) * 32 + (e % 16);
        const u32 w0 = t < T ? R[t * n + tg] : 0u;
        const u32 w1 = t + 16 < T ? R[(t + 16) * n + tg] : 0u;
        isn |= w0 == ST_RANK_NAN || w1 == ST_RANK_NAN;
        Rt[b * (Tp / 2) + e] = (w0 & 0xFFFFu) | ((w1 & 0xFFFFu) << 16);
    }
    if (__syncthreads_or(isn) && threadIdx.x == 0) xnan[b] = 1;
}

// grid = (ceil(n / 256), W32, ceil(nb / ST_TG))
__global__ __launch_bounds__(ST_THREADS) void strict_masks_rank_kernel(
    const u32 *__restrict__ R, const u32 *__restrict__ Rt, i64 T, i64 n, i64 nb, StrictMaskOut o) {
    const i64 cnt = o.dlist ? (i64)*o.dcount : nb;
    const i64 z0 = (i64)blockIdx.z * ST_TG;
    if (z0 >= cnt) return;
    const i64 zend = z0 + ST_TG < cnt ? z0 + ST_TG : cnt;
    const i64 i = (i64)blockIdx.x * ST_THREADS + threadIdx.x;
    const int k = blockIdx.y;
    const int W32 = (int)((T + 31) / 32);
    const i64 t0 = (i64)k * 32;
    const int tl = (int)(T - t0 < 32 ? T - t0 : 32);
    const u32 valid = tl == 32 ? 0xFFFFFFFFu : ((1u << tl) - 1u);
    // two timepoints per register: x2 = rank at t0 + j | rank at t0 + j + 16 << 16 (ranks < 2^15: bit 15 of each half is
    // free), kept as x2 + H and x2 - H (H = 0x80008000) for the two subtractions below
    u32 xh[16], xm[16];
    u32 nanbits = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const u32 w0 = (i < n && j < tl) ? R[(t0 + j) * n + i] : 0u;
        const u32 w1 = (i < n && j + 16 < tl) ? R[(t0 + j + 16) * n + i] : 0u;
        const bool n0 = w0 == ST_RANK_NAN, n1 = w1 == ST_RANK_NAN;
        nanbits |= (n0 ? (1u << j) : 0u) | (n1 ? (1u << (j + 16)) : 0u);
        const u32 x2 = (n0 ? 0u : (w0 & 0xFFFFu)) | ((n1 ? 0u : (w1 & 0xFFFFu)) << 16);
        xh[j] = x2 + 0x80008000u;
        xm[j] = x2 - 0x80008000u;
    }
    // First pass of a matching batch over a full word in which every timepoint counts: only UN is stored, and of DN
    // only "is there a tie" is wanted -- a packed running minimum of x2 ^ q2 (a zero half = equal ranks = a tie)
    // instead of the second subtract / rotate / insert: 2.5 instead of 3 instructions per timepoint.
    // ... and where no two curves of the data set share a value at any timepoint of the word (tiemask: continuous data,
    // everywhere) not even that: 1.5 instructions per timepoint.
    const bool un_only = o.dflag != nullptr && tl == 32 && o.cmask[k] == 0;
    const bool no_ties = un_only && o.tiemask != nullptr && o.tiemask[k] == 0;
    // Both halves at once with plain 32-bit subtractions: each half of (q2 + H) - x2 = q2 - (x2 - H) is
    // q + 0x8000 - x > 0 (no borrow between the halves) and its bit 15 says x <= q; likewise (x2 + H) - q2 for
    // x >= q.  The accumulators rotate right by one per step and take the two bits at 15 and 31 (v_bfi): after 16
    // steps timepoint j sits in bit j and j + 16 in bit 16 + j.  1.5 full-rate instructions per (timepoint,
    // direction); the accumulated sense is inverted (NOT above / NOT below).
    // The next target's 16 rank pairs are fetched (one s_load_dwordx16) while this one's are used: the kernel was
    // waiting on that scalar load for half of its cycles (SQ_WAIT_INST_ANY 0.55 of the wave cycles).
    typedef u32 u32x16 __attribute__((ext_vector_type(16)));
    const u32 H = 0x80008000u;
    // Round 3, after the instruction costs were measured (tools/experiments/valu_rate.hip): v_alignbit_b32 and v_bfi_b32 issue in
    // 4.1 cycles each, v_and_b32 / v_lshrrev_b32 / v_or_b32 in 2.0 - 2.1.  The accumulator starts at 0 and each half is a 16-bit
    // shift register that is full after exactly 16 steps, so a plain 32-bit shift never carries a set bit from the upper half
    // into bit 15: shift, mask, or -- three two-cycle instructions (6.2 cycles) instead of rotate + insert (8.2).
#define ST_SHIFT_IN(acc, d) asm("v_lshrrev_b32 %0, 1, %0\n\tv_and_b32 %1, %2, %1\n\tv_or_b32 %0, %0, %1" : "+v"(acc), "+v"(d) : "s"(H))
    i64 b = o.dlist ? (i64)o.dlist[z0] : z0;
    u32x16 qv = *reinterpret_cast<const u32x16 *>(Rt + (b * W32 + k) * 16);
    for (i64 z = z0; z < zend; ++z) {
        const i64 bn = z + 1 < zend ? (o.dlist ? (i64)o.dlist[z + 1] : z + 1) : b;
        const u32x16 qn = *reinterpret_cast<const u32x16 *>(Rt + (bn * W32 + k) * 16);
        u32 na = 0, nb_ = 0;
        if (no_ties) {                                                  // block-uniform
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                u32 d1 = qv[j] - xm[j];                                 // (q + 0x8000) - x per half; bit 15 / 31: x <= q
                ST_SHIFT_IN(na, d1);
            }
            if (i < n) {
                o.m32[((size_t)b * 2 * W32 + k) * n + i] = ~na | nanbits;
                if (nanbits) o.dflag[(size_t)b * n + i] = 1;
            }
        } else if (un_only) {                                           // block-uniform
            typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
            u16x2 mn = {0xFFFF, 0xFFFF};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const u32 q2 = qv[j];
                u32 d1 = q2 - xm[j];                                    // (q + 0x8000) - x per half; bit 15 / 31: x <= q
                ST_SHIFT_IN(na, d1);
                const u32 e = (xh[j] ^ H) ^ q2;                         // x2 ^ q2 (xh = x2 | H)
                mn = __builtin_elementwise_min(mn, __builtin_bit_cast(u16x2, e));
            }
            const u32 un = ~na | nanbits;
            if (i < n) {
                o.m32[((size_t)b * 2 * W32 + k) * n + i] = un;
                if (mn.x == 0 || mn.y == 0 || nanbits) o.dflag[(size_t)b * n + i] = 1;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const u32 q2 = qv[j];
                u32 d1 = q2 - xm[j];                                    // (q + 0x8000) - x per half; bit 15 / 31: x <= q
                u32 d2 = xh[j] - q2;                                    // (x + 0x8000) - q per half; bit 15 / 31: x >= q
                // rotate right by one, then take bits 15 and 31 from the difference (the compiler's own rendering of
                // this costs a third instruction)
                ST_SHIFT_IN(na, d1);
                ST_SHIFT_IN(nb_, d2);
            }
            strict_store_masks(o, b, k, W32, n, i, (~na | nanbits) & valid, (~nb_ | nanbits) & valid, valid);
        }
        qv = qn;
        b = bn;
    }
}

// ---------------------------------------------------------------------------------------------------
// The same masks from 32-BIT ranks (32 767 < n <= 131 071: config 3's size).  R[t][i] = the large-n route's B word
// (mbd_rank_big.hip, launch_rank_big_image): curves strictly below curve i at t, bit 31 set when the curve ties with
// another one there, 0xFFFFFFFF for NaN.  B is order- and tie-preserving, so x_i > x_q <=> B_i > B_q <=> bit 31 of
// B_q - B_i (ranks < 2^31): v_sub_u32 + v_alignbit_b32 per (timepoint, direction) against two half-rate v_cmp_f64 +
// two v_cndmask + v_or of the fp64 kernel.  Thread = curve, block = 256 curves x one word x 32 targets, as above.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS) void strict_row_ties32_kernel(const u32 *__restrict__ R, i64 n, u32 *__restrict__ tiemask) {
    const i64 t = blockIdx.x;
    bool tie = false;
    for (i64 i = threadIdx.x; i < n; i += ST_THREADS) {
        const u32 w = R[t * n + i];
        tie |= w != ST_RANK_NAN && (w >> 31) != 0;
    }
    if (__syncthreads_or(tie) && threadIdx.x == 0) atomicOr(&tiemask[t >> 5], 1u << (t & 31));
}

// Rt[b][t] = the target's rank at t (tie bit cleared; 0 beyond T and for NaN, which is noted in xnan)
__global__ __launch_bounds__(ST_THREADS) void strict_gather_rank32_targets_kernel(
    const u32 *__restrict__ R, i64 T, i64 n, const i64 *__restrict__ targets, i64 q0, u32 *__restrict__ Rt,
    u32 *__restrict__ xnan) {
    const i64 b = blockIdx.x;
    const i64 tg = targets ? targets[q0 + b] : q0 + b;
    const i64 Tp = ((T + 31) / 32) * 32;
    bool isn = false;
    for (i64 t = threadIdx.x; t < Tp; t += ST_THREADS) {
        const u32 w = t < T ? R[t * n + tg] : 0u;
        isn |= w == ST_RANK_NAN;
        Rt[b * Tp + t] = w == ST_RANK_NAN ? 0u : (w & 0x7FFFFFFFu);
    }
    if (__syncthreads_or(isn) && threadIdx.x == 0) xnan[b] = 1;
}

// grid = (ceil(n / 256), W32, ceil(nb / ST_TG))
__global__ __launch_bounds__(ST_THREADS) void strict_masks_rank32_kernel(
    const u32 *__restrict__ R, const u32 *__restrict__ Rt, i64 T, i64 n, i64 nb, StrictMaskOut o) {
    const i64 cnt = o.dlist ? (i64)*o.dcount : nb;
    const i64 z0 = (i64)blockIdx.z * ST_TG;
    if (z0 >= cnt) return;
    const i64 zend = z0 + ST_TG < cnt ? z0 + ST_TG : cnt;
    const i64 i = (i64)blockIdx.x * ST_THREADS + threadIdx.x;
    const int k = blockIdx.y;
    const int W32 = (int)((T + 31) / 32);
    const i64 t0 = (i64)k * 32;
    const int tl = (int)(T - t0 < 32 ? T - t0 : 32);
    const u32 valid = tl == 32 ? 0xFFFFFFFFu : ((1u << tl) - 1u);
    u32 x[32];
    u32 nanbits = 0;
#pragma unroll
    for (int t = 0; t < 32; ++t) {
        const u32 w = (i < n && t < tl) ? R[(t0 + t) * n + i] : 0u;
        const bool isn = w == ST_RANK_NAN;
        nanbits |= isn ? (1u << t) : 0u;
        x[t] = isn ? 0u : (w & 0x7FFFFFFFu);
    }
    const bool un_only = o.dflag != nullptr && tl == 32 && o.cmask[k] == 0;
    const bool no_ties = un_only && o.tiemask != nullptr && o.tiemask[k] == 0;
    typedef u32 u32x16 __attribute__((ext_vector_type(16)));
    for (i64 z = z0; z < zend; ++z) {
        const i64 b = o.dlist ? (i64)o.dlist[z] : z;
        const u32 *qp = Rt + (b * W32 + k) * 32;                      // wave-uniform: two s_load_dwordx16
        const u32x16 qa = *reinterpret_cast<const u32x16 *>(qp), qb = *reinterpret_cast<const u32x16 *>(qp + 16);
        u32 un = 0, dn = 0;
        if (no_ties) {                                                // block-uniform: continuous data, everywhere
#pragma unroll
            for (int t = 31; t >= 0; --t) un = __builtin_amdgcn_alignbit(un, (t < 16 ? qa[t] : qb[t - 16]) - x[t], 31);
            if (i < n) {
                o.m32[((size_t)b * 2 * W32 + k) * n + i] = un | nanbits;
                if (nanbits) o.dflag[(size_t)b * n + i] = 1;
            }
        } else if (un_only) {                                         // block-uniform: of DN only "is there a tie" is wanted
            u32 mn = 0xFFFFFFFFu;
#pragma unroll
            for (int t = 31; t >= 0; --t) {
                const u32 q = t < 16 ? qa[t] : qb[t - 16];
                un = __builtin_amdgcn_alignbit(un, q - x[t], 31);
                const u32 e = q ^ x[t];
                mn = mn < e ? mn : e;
            }
            if (i < n) {
                o.m32[((size_t)b * 2 * W32 + k) * n + i] = un | nanbits;
                if (mn == 0u || nanbits) o.dflag[(size_t)b * n + i] = 1;
            }
        } else {
#pragma unroll
            for (int t = 31; t >= 0; --t) {
                const u32 q = t < 16 ? qa[t] : qb[t - 16];
                un = __builtin_amdgcn_alignbit(un, q - x[t], 31);     // x above q
                dn = __builtin_amdgcn_alignbit(dn, x[t] - q, 31);     // x below q
            }
            strict_store_masks(o, b, k, W32, n, i, (un | nanbits) & valid, (dn | nanbits) & valid, valid);
        }
    }
}

// What the complement matching below needs per (target, curve), read off the UN masks once:
//   HF[b][i] = payload (60 bits) << 4 | exact << 3 | side << 2 | canonical mask non-empty << 1 | clean
// payload: the canonical mask itself when it has one non-zero word (exact = 1: word index << 32 | word), else 60 hash bits
// (canonical form, side, clean: see the matching section; cmask marks the timepoints that do not count).
// grid = (ceil(n / 256), nb); the words of a curve are n apart (word-major image): every load is coalesced.
// (Folding this into the mask kernel was measured: carrying 8 or 16 targets' hashes in VGPRs across all words costs
// the occupancy and the 32-target reuse of the curve values that strict_masks2_kernel lives on -- 30 and 47 ms instead
// of 17.6 + 6 ms at 10 000 x 1 000.)
__device__ __forceinline__ u64 strict_mix(u64 h, u32 w) {
    h = (h ^ w) * 0xff51afd7ed558ccdull;
    return h ^ (h >> 29);
}

struct StrictFirst {            // the first timepoint that counts: word and bit (wave-uniform)
    int wf;
    u32 vf;
};
__device__ __forceinline__ StrictFirst strict_first_counting(const u32 *__restrict__ cmask, int W32, u32 lastvalid) {
    StrictFirst f{0, 0u};
    for (; f.wf < W32; ++f.wf) {
        f.vf = (f.wf == W32 - 1 ? lastvalid : 0xFFFFFFFFu) & ~cmask[f.wf];
        if (f.vf) break;
    }
    return f;
}

__global__ __launch_bounds__(ST_THREADS) void strict_hash_kernel(const u32 *__restrict__ m32, i64 T, i64 n,
                                                                const u32 *__restrict__ xnan, const u32 *__restrict__ cmask,
                                                                const unsigned char *__restrict__ dflag, u64 *__restrict__ HF) {
    const i64 b = blockIdx.y;
    if (xnan[b]) return;
    const i64 a = (i64)blockIdx.x * ST_THREADS + threadIdx.x;
    if (a >= n) return;
    const int W32 = (int)((T + 31) / 32);
    const u32 lastvalid = (T & 31) ? ((1u << (T & 31)) - 1u) : 0xFFFFFFFFu;
    const u32 *mb = m32 + (size_t)b * 2 * W32 * n;
    const StrictFirst fc = strict_first_counting(cmask, W32, lastvalid);
    // dirty (tie / NaN where it counts): noted by the mask kernel; every row constant: nothing is clean (pair kernel)
    const bool clean = fc.vf != 0 && dflag[(size_t)b * n + a] == 0;
    u32 side = 0, flip = 0;
    if (fc.vf) {
        side = (mb[(size_t)fc.wf * n + a] >> (__ffs((int)fc.vf) - 1)) & 1u;
        flip = side ? 0xFFFFFFFFu : 0u;
    }
    u64 h = 0x9E3779B97F4A7C15ull;
    u32 one = 0, onek = 0, nz = 0;                            // the only non-zero canonical word, its index, how many there are
    for (int w0 = 0; w0 < W32; w0 += 16) {
        u32 un[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {                        // sixteen loads in flight
            const int w = w0 + j < W32 ? w0 + j : W32 - 1;
            un[j] = mb[(size_t)w * n + a];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int w = w0 + j;
            if (w < W32) {
                const u32 v = (w == W32 - 1 ? lastvalid : 0xFFFFFFFFu) & ~cmask[w];
                const u32 cw = (un[j] ^ flip) & v;
                if (cw) { one = cw; onek = (u32)w; ++nz; }
                h = strict_mix(h, cw);
            }
        }
    }
    // a canonical mask with a single non-zero word is described EXACTLY by (index, word): equal payloads are equal
    // masks and need no look at the masks (most groups of real data: curves that cross the target within one stretch
    // of 32 timepoints and stay on one side otherwise)
    const bool exact = nz <= 1;
    u64 payload;
    if (exact) {
        payload = ((u64)onek << 32) | one;
    } else {
        h ^= h >> 32;
        h *= 0xc4ceb9fe1a85ec53ull;
        h ^= h >> 33;
        payload = h >> 4;
    }
    HF[(size_t)b * n + a] = (payload << 4) | ((exact ? 1u : 0u) << 3) | (side << 2) | ((nz ? 1u : 0u) << 1) | (clean ? 1u : 0u);
}

// one (a tile, b chunk) of target b; db = the target's dirty bitmap when matching has counted the clean-clean pairs
__device__ __forceinline__ void strict_pairs2_target(const u32 *__restrict__ m32, i64 T, i64 n, const i64 *__restrict__ targets,
                                                     i64 q0, const u64 *__restrict__ dbits, u64 *__restrict__ out, int jcols,
                                                     const i64 b) {
    __shared__ u64 scratch[ST_THREADS / 64];
    __shared__ u32 orparts[ST_THREADS / 64][2][ST_SUB];   // per wave: OR of its quarter of partner j's UN / DN words
    __shared__ __attribute__((aligned(16))) u32 cm[ST_SUB][2 * ST_W32 + 4];   // partner j: UN words 0..31, DN words 0..31 (zero
                                                                                // beyond W32); rows padded by 16 bytes: the survivors'
                                                                                // per-lane rows fall on different banks
    const i64 q = q0 + b;
    // with matching on, the pairs of two clean curves are counted there; here only pairs with a dirty member remain
    const u64 *db = dbits ? dbits + (size_t)b * ((n + 63) / 64) : nullptr;
    const i64 tg = targets ? targets[q] : q;
    const i64 a = (i64)blockIdx.x * ST_THREADS + threadIdx.x;
    const i64 b0 = (i64)blockIdx.y * ST_BCHUNK;
    const i64 b1 = b0 + ST_BCHUNK < n ? b0 + ST_BCHUNK : n;
    const i64 amin = (i64)blockIdx.x * ST_THREADS;
    if (b1 - 1 <= amin) return;                // whole chunk at or below the tile: no a < b pair
    const int W32 = (int)((T + 31) / 32);
    const u32 *mb = m32 + (size_t)b * 2 * W32 * n;
    const bool alive = a < n && a != tg;
    u32 un[ST_W32], dn[ST_W32];
#pragma unroll
    for (int w = 0; w < ST_W32; ++w) {
        un[w] = (alive && w < W32) ? mb[(size_t)w * n + a] : 0u;
        dn[w] = (alive && w < W32) ? mb[(size_t)(W32 + w) * n + a] : 0u;
    }
    // a curve that is never above the target (UN empty) cannot conflict with one that is never below it (DN empty):
    // such pairs -- most of the contained pairs of banded data -- need no walk over the masks
    u32 ora = 0, ord_ = 0;
#pragma unroll
    for (int w = 0; w < ST_W32; ++w) { ora |= un[w]; ord_ |= dn[w]; }
    const bool u0a = ora == 0, d0a = ord_ == 0;
    const bool dirty_a = !db || (alive && ((db[a >> 6] >> (a & 63)) & 1));
    const bool tile_dirty = __syncthreads_or(dirty_a) != 0;     // block-uniform
    u64 good = 0;
    for (i64 s0 = b0; s0 < b1; s0 += ST_SUB) {
        const int len = (int)(b1 - s0 < ST_SUB ? b1 - s0 : ST_SUB);
        const u64 dsub = db ? db[s0 >> 6] : ~0ull;              // dirty partners of this sub-chunk (s0 is a multiple of 64)
        if (!tile_dirty && dsub == 0) continue;                 // clean tile x clean partners: nothing to count here
        __syncthreads();                                        // the previous sub-chunk has been read
        for (int e = threadIdx.x; e < ST_SUB * 2 * ST_W32; e += ST_THREADS) {
            const int w2 = e / ST_SUB, j = e % ST_SUB;          // consecutive threads: consecutive partners of one word
            const int w = w2 % ST_W32;
            u32 v = 0;
            if (j < len && w < W32) v = mb[(size_t)(w2 < ST_W32 ? w : W32 + w) * n + s0 + j];
            cm[j][w2] = v;
        }
        __syncthreads();
        // which partners have an empty UN / DN mask: wave w ORs words 8w..8w+7 of partner j = lane, the four waves meet in LDS
        {
            const int j = threadIdx.x & 63, part = threadIdx.x >> 6;
            u32 pu = 0, pd = 0;
#pragma unroll
            for (int w = 0; w < 8; w += 4) {
                const uint4 cu = *reinterpret_cast<const uint4 *>(&cm[j][part * 8 + w]);
                const uint4 cd = *reinterpret_cast<const uint4 *>(&cm[j][ST_W32 + part * 8 + w]);
                pu |= cu.x | cu.y | cu.z | cu.w;
                pd |= cd.x | cd.y | cd.z | cd.w;
            }
            orparts[part][0][j] = pu;
            orparts[part][1][j] = pd;
        }
        __syncthreads();
        u64 U0, D0;                                             // bit j: partner j has no UN / no DN bit (wave-uniform)
        {
            const int j = threadIdx.x & 63;
            U0 = __ballot((orparts[0][0][j] | orparts[1][0][j] | orparts[2][0][j] | orparts[3][0][j]) == 0);
            D0 = __ballot((orparts[0][1][j] | orparts[1][1][j] | orparts[2][1][j] | orparts[3][1][j]) == 0);
        }
        // ---- pass 1: first four words of every partner; survivors as bits ----
        u64 surv = 0;
#pragma unroll 8
        for (int j = 0; j < ST_SUB; ++j) {
            const uint4 cu = *reinterpret_cast<const uint4 *>(&cm[j][0]);
            const uint4 cd = *reinterpret_cast<const uint4 *>(&cm[j][ST_W32]);
            const u32 bad = (un[0] & cu.x) | (un[1] & cu.y) | (un[2] & cu.z) | (un[3] & cu.w) | (dn[0] & cd.x) |
                            (dn[1] & cd.y) | (dn[2] & cd.z) | (dn[3] & cd.w);
            surv |= (u64)(bad == 0) << j;
        }
        // real partners only (a curve that ties with the target everywhere has empty masks and conflicts with nothing,
        // not even with the padding or the target's own slot): block-uniform mask; then c > a only
        u64 real = len == ST_SUB ? ~0ull : (((u64)1 << len) - 1);
        if (tg >= s0 && tg < s0 + len) real &= ~((u64)1 << (int)(tg - s0));
        surv = alive ? (surv & real) : 0;
        if (!dirty_a) surv &= dsub;
        const i64 jf = a + 1 - s0;
        surv = (jf <= 0) ? surv : (jf >= 64 ? 0 : (surv >> (int)jf) << (int)jf);
        if (W32 <= 4) {
            good += (u64)__popcll(surv);
        } else {
            // pairs that cannot conflict by class: counted without the walk
            const u64 sure = surv & ((u0a ? D0 : 0ull) | (d0a ? U0 : 0ull));
            good += (u64)__popcll(sure);
            surv &= ~sure;
            // ---- pass 2: the survivors' remaining words ----
            while (surv) {
                const int j = __ffsll((long long)surv) - 1;
                surv &= surv - 1;
                u32 bad = 0;
#pragma unroll
                for (int w = 4; w < ST_W32; w += 4) {                   // 16-byte LDS reads (per-lane partner j)
                    const uint4 cu = *reinterpret_cast<const uint4 *>(&cm[j][w]);
                    const uint4 cd = *reinterpret_cast<const uint4 *>(&cm[j][ST_W32 + w]);
                    bad |= (un[w] & cu.x) | (un[w + 1] & cu.y) | (un[w + 2] & cu.z) | (un[w + 3] & cu.w) | (dn[w] & cd.x) |
                           (dn[w + 1] & cd.y) | (dn[w + 2] & cd.z) | (dn[w + 3] & cd.w);
                }
                good += (bad == 0);
            }
        }
    }
    u64 tot = block_sum(good, scratch);
    if (threadIdx.x == 0 && tot) atomicAdd(&out[q * jcols], tot);
}

// The same count over the target's LIST of curves that can be in a pair the matching has not counted (strict_match_lds_kernel
// writes it): the dirty curves (ties / NaN with the target; bit 31 of their entry) and the clean curves that cross the target.
// A clean curve that stays below (above) the target throughout contains it with a dirty curve a exactly when a is never
// below (never above) it -- DN_a (UN_a) empty -- so those partners, the bulk of banded or quantised data, are counted as
// z0 (z1) per dirty curve without a look at their masks.  ilist[b]: {entries, z0, z1, -, entry...}; the a < c rule runs
// on list positions.
// Tiles of ST_P3_THREADS = 1 024 list positions, each walking the WHOLE list: a partner sub-chunk is staged once per 1 024 lanes
// and a lane's own masks are fetched once per target (staging was half of the 256-thread, 512-partner form's time).
constexpr int ST_P3_THREADS = 1024;
__device__ __forceinline__ void strict_pairs3_target(const u32 *__restrict__ m32, i64 T, i64 n, i64 q0,
                                                     const u32 *__restrict__ ilist, u64 *__restrict__ out, int jcols,
                                                     const i64 b, const int tile, const int chunk, const int chunks) {
    __shared__ u64 scratch[ST_P3_THREADS / 64];
    __shared__ u32 orparts[4][2][ST_SUB];   // per wave: OR of its quarter of partner j's UN / DN words
    __shared__ __attribute__((aligned(16))) u32 cm[ST_SUB][2 * ST_W32 + 4];   // partner j: UN words 0..31, DN words 0..31 (zero
                                                                                // beyond W32); rows padded by 16 bytes: the survivors'
                                                                                // per-lane rows fall on different banks
    __shared__ u32 sidx[ST_SUB];                            // the sub-chunk's curve indices (bit 31: dirty)
    const i64 q = q0 + b;
    const u32 *lst = ilist + (size_t)b * (n + 4);
    const i64 nd_l = (i64)lst[0], nc_l = (i64)lst[3];          // dirty entries first, then the clean ones (stored from the back)
    const i64 len_l = nd_l + nc_l;
    const u64 z0 = lst[1], z1 = lst[2];
    lst += 4;
    auto entry = [&](i64 pos) -> u32 { return pos < nd_l ? lst[pos] : lst[n - 1 - (pos - nd_l)]; };
    const i64 apos = (i64)tile * ST_P3_THREADS + threadIdx.x;
    const i64 amin = (i64)tile * ST_P3_THREADS;
    if (amin >= nd_l) return;                               // a tile without a dirty lane: every pair of its lanes with a dirty
                                                            // curve is counted by that curve's lane (the earlier position)
    // This block's share of the partners.  A tile with many dirty lanes walks the whole list itself (one staging per 1 024
    // lanes, its masks fetched once); a few dirty lanes against a long list (a handful of ties in continuous data) are
    // latency-bound on one block, so the list is cut into `chunks` pieces that run side by side.
    const i64 dirty_here = nd_l - amin < ST_P3_THREADS ? nd_l - amin : ST_P3_THREADS;
    const i64 nchunk = dirty_here >= 128 ? 1 : (i64)chunks;
    const i64 csz = ((len_l + nchunk - 1) / nchunk + ST_SUB - 1) / ST_SUB * ST_SUB;
    if ((i64)chunk >= nchunk) return;
    const i64 b0 = (i64)chunk * csz;
    const i64 b1 = b0 + csz < len_l ? b0 + csz : len_l;
    const bool closed = chunk == 0;                   // this block also adds its lanes' pairs with the z0 / z1 curves
    if ((b0 >= len_l || b1 - 1 <= amin) && !closed) return;   // no partner here, or the whole chunk at or below the tile
    const int W32 = (int)((T + 31) / 32);
    const u32 *mb = m32 + (size_t)b * 2 * W32 * n;
    const bool alive = apos < len_l;
    const u32 ent = alive ? entry(apos) : 0u;
    const i64 a = (i64)(ent & 0x7FFFFFFFu);
    u32 un[ST_W32], dn[ST_W32];
#pragma unroll
    for (int w = 0; w < ST_W32; ++w) {
        un[w] = (alive && w < W32) ? mb[(size_t)w * n + a] : 0u;
        dn[w] = (alive && w < W32) ? mb[(size_t)(W32 + w) * n + a] : 0u;
    }
    // a curve that is never above the target (UN empty) cannot conflict with one that is never below it (DN empty):
    // such pairs -- most of the contained pairs of banded data -- need no walk over the masks
    u32 ora = 0, ord_ = 0;
#pragma unroll
    for (int w = 0; w < ST_W32; ++w) { ora |= un[w]; ord_ |= dn[w]; }
    const bool u0a = ora == 0, d0a = ord_ == 0;
    const bool dirty_a = alive && (ent >> 31);
    const bool tile_dirty = __syncthreads_or(dirty_a) != 0;     // block-uniform
    u64 good = 0;
    if (closed && dirty_a) good += (d0a ? z0 : 0ull) + (u0a ? z1 : 0ull);
    for (i64 s0 = b0; s0 < b1; s0 += ST_SUB) {
        if (s0 + ST_SUB <= amin + 1) continue;                  // every partner of this sub-chunk at or below every lane's position
        const int len = (int)(b1 - s0 < ST_SUB ? b1 - s0 : ST_SUB);
        __syncthreads();                                        // the previous sub-chunk has been read
        if (threadIdx.x < ST_SUB) sidx[threadIdx.x] = threadIdx.x < len ? entry(s0 + threadIdx.x) : 0u;
        __syncthreads();
        const u64 dsub = __ballot((int)(threadIdx.x & 63) < len && (sidx[threadIdx.x & 63] >> 31));   // dirty partners of this sub-chunk
        if (!tile_dirty && dsub == 0) continue;                 // clean tile x clean partners: counted by the matching
        for (int e = threadIdx.x; e < ST_SUB * 2 * ST_W32; e += ST_P3_THREADS) {
            const int w2 = e / ST_SUB, j = e % ST_SUB;          // consecutive threads: consecutive partners of one word
            const int w = w2 % ST_W32;
            u32 v = 0;
            if (j < len && w < W32) v = mb[(size_t)(w2 < ST_W32 ? w : W32 + w) * n + (sidx[j] & 0x7FFFFFFFu)];
            cm[j][w2] = v;
        }
        __syncthreads();
        // which partners have an empty UN / DN mask: wave w ORs words 8w..8w+7 of partner j = lane, the four waves meet in LDS
        if (threadIdx.x < 256) {
            const int j = threadIdx.x & 63, part = threadIdx.x >> 6;
            u32 pu = 0, pd = 0;
#pragma unroll
            for (int w = 0; w < 8; w += 4) {
                const uint4 cu = *reinterpret_cast<const uint4 *>(&cm[j][part * 8 + w]);
                const uint4 cd = *reinterpret_cast<const uint4 *>(&cm[j][ST_W32 + part * 8 + w]);
                pu |= cu.x | cu.y | cu.z | cu.w;
                pd |= cd.x | cd.y | cd.z | cd.w;
            }
            orparts[part][0][j] = pu;
            orparts[part][1][j] = pd;
        }
        __syncthreads();
        u64 U0, D0;                                             // bit j: partner j has no UN / no DN bit (wave-uniform)
        {
            const int j = threadIdx.x & 63;
            U0 = __ballot((orparts[0][0][j] | orparts[1][0][j] | orparts[2][0][j] | orparts[3][0][j]) == 0);
            D0 = __ballot((orparts[0][1][j] | orparts[1][1][j] | orparts[2][1][j] | orparts[3][1][j]) == 0);
        }
        // ---- pass 1: first four words of every partner; survivors as bits ----
        u64 surv = 0;
#pragma unroll 8
        for (int j = 0; j < ST_SUB; ++j) {
            const uint4 cu = *reinterpret_cast<const uint4 *>(&cm[j][0]);
            const uint4 cd = *reinterpret_cast<const uint4 *>(&cm[j][ST_W32]);
            const u32 bad = (un[0] & cu.x) | (un[1] & cu.y) | (un[2] & cu.z) | (un[3] & cu.w) | (dn[0] & cd.x) |
                            (dn[1] & cd.y) | (dn[2] & cd.z) | (dn[3] & cd.w);
            surv |= (u64)(bad == 0) << j;
        }
        // real partners only (a curve that ties with the target everywhere has empty masks and conflicts with nothing,
        // not even with the padding or the target's own slot): block-uniform mask; then c > a only
        const u64 real = len == ST_SUB ? ~0ull : (((u64)1 << len) - 1);
        surv = alive ? (surv & real) : 0;
        if (!dirty_a) surv &= dsub;
        const i64 jf = apos + 1 - s0;
        surv = (jf <= 0) ? surv : (jf >= 64 ? 0 : (surv >> (int)jf) << (int)jf);
        if (W32 <= 4) {
            good += (u64)__popcll(surv);
        } else {
            // pairs that cannot conflict by class: counted without the walk
            const u64 sure = surv & ((u0a ? D0 : 0ull) | (d0a ? U0 : 0ull));
            good += (u64)__popcll(sure);
            surv &= ~sure;
            // ---- pass 2: the survivors' remaining words ----
            while (surv) {
                const int j = __ffsll((long long)surv) - 1;
                surv &= surv - 1;
                u32 bad = 0;
#pragma unroll
                for (int w = 4; w < ST_W32; w += 4) {                   // 16-byte LDS reads (per-lane partner j)
                    const uint4 cu = *reinterpret_cast<const uint4 *>(&cm[j][w]);
                    const uint4 cd = *reinterpret_cast<const uint4 *>(&cm[j][ST_W32 + w]);
                    bad |= (un[w] & cu.x) | (un[w + 1] & cu.y) | (un[w + 2] & cu.z) | (un[w + 3] & cu.w) | (dn[w] & cd.x) |
                           (dn[w + 1] & cd.y) | (dn[w + 2] & cd.z) | (dn[w + 3] & cd.w);
                }
                good += (bad == 0);
            }
        }
    }
    u64 tot = block_sum(good, scratch);
    if (threadIdx.x == 0 && tot) atomicAdd(&out[q * jcols], tot);
}

// Without matching: grid = (a tiles, b chunks, nb), block z = target z.  With matching: grid.z is a fixed number of
// layers that share out the batch's targets WITH dirty curves (dlist, *dcount: appended by the matching kernels) --
// continuous data has none, and a grid over all targets would cost more in empty blocks than everything else here.
constexpr int ST_PAIR_LAYERS = 32;
__global__ __launch_bounds__(ST_THREADS) void strict_pairs2_kernel(
    const u32 *__restrict__ m32, i64 T, i64 n, const i64 *__restrict__ targets, i64 q0,
    const u32 *__restrict__ xnan, const u32 *__restrict__ dlist, const u32 *__restrict__ dcount,
    const u64 *__restrict__ dbits, u64 *__restrict__ out, int jcols) {
    if (!dlist) {
        if (xnan[blockIdx.z]) return;              // NaN in the target: nothing is contained
        strict_pairs2_target(m32, T, n, targets, q0, nullptr, out, jcols, (i64)blockIdx.z);
        return;
    }
    const u32 cnt = *dcount;
    for (u32 zi = blockIdx.z; zi < cnt; zi += gridDim.z) {
        strict_pairs2_target(m32, T, n, targets, q0, dbits, out, jcols, (i64)dlist[zi]);
        __syncthreads();                           // the target's shared arrays are reused by the next one
    }
}

// A persistent 1-D grid over the items (dirty target of the matching's work list, tile of 1 024 list positions, chunk of
// partners); an item without work (a tile beyond the target's dirty entries, a chunk the tile does not use) costs its block
// a look at the list's header, not a workgroup launch: thousands of 1 024-thread workgroups that return at once cost more
// in the dispatcher than the real ones cost in the kernel (measured: 3.3 -> 5.2 ms at 2 000 x 1 000 for twice the grid).
__global__ __launch_bounds__(ST_P3_THREADS) void strict_pairs3_kernel(
    const u32 *__restrict__ m32, i64 T, i64 n, i64 q0, const u32 *__restrict__ dlist, const u32 *__restrict__ dcount,
    const u32 *__restrict__ ilist, u64 *__restrict__ out, int jcols, int tiles, int chunks) {
    const i64 cnt = (i64)*dcount, items = cnt * tiles * chunks;
    // item = (chunk, tile, target), targets fastest: the items with work (chunk 0 of the first tiles of every target) are
    // consecutive and spread evenly over the blocks
    for (i64 it = blockIdx.x; it < items; it += gridDim.x) {
        const i64 zi = it % cnt;
        const int rem = (int)(it / cnt);
        strict_pairs3_target(m32, T, n, q0, ilist, out, jcols, (i64)dlist[zi], rem % tiles, rem / tiles, chunks);
        __syncthreads();                           // the item's shared arrays are reused by the next one
    }
}

// ---------------------------------------------------------------------------------------------------
// J = 2 by complement matching: O(n T) per target instead of O(n^2 T).
// Call a curve CLEAN for a target when at every timepoint that counts it is strictly above or strictly below it (no
// tie, no NaN): DN = ~UN.  A pair of clean curves is contained at every timepoint iff at every timepoint exactly one
// of them is above, i.e. iff UN_b == ~UN_a as T-bit masks: an EQUALITY, so the pairs can be counted by grouping
// instead of testing.  Canonical form of a mask: itself (side 0) or its complement (side 1), whichever is 0 at the
// first timepoint that counts; complementary masks share their canonical form and sit on opposite sides, so
//     clean-clean contained pairs = sum over distinct canonical masks of  count(side 0) * count(side 1).
// The empty canonical mask (curves below / above the target throughout) is counted directly; the others are grouped
// in an open-addressing table per target keyed by a digest of the canonical mask (strict_hash_kernel).  A slot holds hash bits + the id of the first curve that claimed it (one CAS, no lock,
// nothing to wait for); a curve that meets a key with its hash compares its full canonical mask with that first
// curve's before joining, so hash collisions cost a probe and never a wrong count.
// Curves that are not clean (ties, NaN) are DIRTY: pairs with a dirty member are counted by strict_pairs2_kernel,
// which skips everything else (dirty bitmap per target); continuous data has none and the pair kernel exits at once.
// ---------------------------------------------------------------------------------------------------
// Timepoints at which all curves hold the same value (a common start, say) constrain no pair: cmask has their bits, and
// the matching treats them as absent (they would otherwise make every curve "tie" and send every target to the pair
// kernel).
__global__ __launch_bounds__(ST_THREADS) void strict_const_rows_kernel(const double *__restrict__ Y, i64 T, i64 n,
                                                                      u32 *__restrict__ cmask) {
    // grid = T blocks, one per timepoint (cmask zeroed before): a row of equal values sets its bit
    const i64 t = blockIdx.x;
    const double *row = Y + t * n;
    const double first = row[0];
    bool differs = false;
    for (i64 i0 = 0; i0 < n; i0 += (i64)ST_THREADS * 8) {       // eight strides between the block-wide checks
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const i64 i = i0 + (i64)u * ST_THREADS + threadIdx.x;
            if (i < n && !(row[i] == first)) differs = true;     // NaN differs from everything
        }
        if (__syncthreads_or(differs)) return;                   // block-uniform
    }
    if (threadIdx.x == 0) atomicOr(&cmask[t >> 5], 1u << (t & 31));
}

// do curves a and rep have the same canonical mask for this target?  Equal HF words (payload, exact flag; sides apart)
// are required; exact payloads settle it, hashed ones (masks spread over several words) are confirmed on the masks.
__device__ __forceinline__ bool strict_same_canonical(const u32 *__restrict__ mb, i64 n, int W32, u32 lastvalid,
                                                      const u32 *__restrict__ cmask, i64 a, u64 hfa, i64 rep, u64 hfr) {
    if ((hfa >> 3) != (hfr >> 3)) return false;
    if (hfa & 8) return true;
    const u32 flip = (hfa & 4) ? 0xFFFFFFFFu : 0u, rflip = (hfr & 4) ? 0xFFFFFFFFu : 0u;
    u32 diff = 0;
    for (int w0 = 0; w0 < W32; w0 += 8) {
        u32 ma[8], mr[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {                         // sixteen loads in flight
            const int w = w0 + j < W32 ? w0 + j : W32 - 1;
            ma[j] = mb[(size_t)w * n + a];
            mr[j] = mb[(size_t)w * n + rep];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int w = w0 + j < W32 ? w0 + j : W32 - 1;
            const u32 v = (w == W32 - 1 ? lastvalid : 0xFFFFFFFFu) & ~cmask[w];
            diff |= ((ma[j] ^ flip) ^ (mr[j] ^ rflip)) & v;
        }
    }
    return diff == 0;
}

// One block per target, the table in LDS (8 bytes per slot: key = 14 tag bits | side | 17-bit id
// of the first curve with that canonical mask; counter = members after the first, side 0 in the low half, side 1 in
// the high half).  A curve that meets its own canonical mask joins the group with one LDS atomic on the counter; the
// value it gets back is the group before it, so `members on the other side so far` summed over the joiners is exactly
// count(side 0) * count(side 1).  Also writes the target's dirty bitmap and count for the pair kernel, and its total.
constexpr i64 ST_MATCH_LDS_CAP = 13107;                       // candidates the LDS table takes: 16 384 slots (128 KiB), load 0.8
constexpr int ST_ML_THREADS = 1024;
constexpr int ST_ML_SEEN = 65536;                             // bits per side of the "digest seen" filter (2 x 8 KiB of LDS)
static inline i64 strict_lds_slots(i64 n) {
    i64 s = 64;
    while (s * 4 < n * 5 && s < 16384) s <<= 1;
    return s;
}
__device__ __forceinline__ u64 strict_spread(u64 hf) {        // slot and tag bits from the payload (exact ones are not hashed yet)
    u64 h = (hf >> 3) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 31);
}
__global__ __launch_bounds__(ST_ML_THREADS) void strict_match_lds_kernel(
    const u32 *__restrict__ m32, const u64 *__restrict__ HF, i64 T, i64 n, const i64 *__restrict__ targets, i64 q0,
    const u32 *__restrict__ xnan, const u32 *__restrict__ cmask, u32 *__restrict__ meta, u64 *__restrict__ dbits,
    u32 *__restrict__ dlist, u32 *__restrict__ dcount, int slots, int whole_targets, int force_overflow,
    u64 *__restrict__ out, int jcols, u32 *__restrict__ ilist) {
    extern __shared__ u32 tabl[];                             // keys [slots] | counters [slots]
    __shared__ u64 red[ST_ML_THREADS / 64][3];
    __shared__ u32 lcount, ccount;                            // the pair kernel's curve list so far: dirty entries (from the front), clean ones (from the back)
    const i64 b = blockIdx.x;
    if (xnan[b]) return;
    const i64 tg = targets ? targets[q0 + b] : q0 + b;
    const int tid = threadIdx.x;
    const int W32 = (int)((T + 31) / 32);
    const u32 lastvalid = (T & 31) ? ((1u << (T & 31)) - 1u) : 0xFFFFFFFFu;
    const u32 *mb = m32 + (size_t)b * 2 * W32 * n;
    const u64 *hb = HF + (size_t)b * n;
    u32 *cntl = tabl + slots;
    u32 *seen = cntl + slots;                                 // [2][ST_ML_SEEN / 32]: digests present on side 0 / side 1
    for (int e = tid; e < 2 * slots + 2 * (ST_ML_SEEN / 32); e += ST_ML_THREADS) tabl[e] = 0;
    if (tid == 0) { lcount = 0; ccount = 0; }
    u32 *lst = ilist ? ilist + (size_t)b * (n + 4) + 4 : nullptr;
    __syncthreads();
    u64 acc = 0;
    u32 z0 = 0, z1 = 0, nd = 0;
    // More curves than the table takes at a load of 0.8 (n > 13 107: slots = 16 384): the 2 x 8 KiB filter would fill up
    // (at n = 10^5 half of the crossing curves passed it and the table was filled in 5 - 6 rounds, every round a pass over the
    // digests: 0.52 of config-3-size's 0.83 s).  Then the whole table area serves as the filter first -- 2^19 bits per
    // side, load < 0.13 -- the few curves that pass it are remembered as one bit per (thread, iteration) in registers, and
    // the table is built from them alone: three passes over the digests, no rounds.
    const bool must_count = (i64)n * 5 > (i64)slots * 4;
    const bool bigf = must_count && slots == 16384;                         // block-uniform
    u32 *fbits = bigf ? tabl : seen;                                        // [2][FB / 32]
    const u32 FB = bigf ? (1u << 19) : (u32)ST_ML_SEEN;
    // Pass 1: dirty curves, the two empty-mask counts, and one bit per (side, digest): a curve can only pair with a
    // curve whose canonical mask -- hence digest -- it shares on the OTHER side, and in continuous data hardly any
    // digest occurs on both sides.  One LDS atomic per curve, no probing.
    for (i64 a0 = 0; a0 < n; a0 += ST_ML_THREADS) {
        const i64 a = a0 + tid;
        const bool active = a < n && a != tg;
        const u64 hf = a < n ? hb[a] : 0;
        const bool clean = hf & 1;
        const u32 side = (u32)(hf >> 2) & 1u;
        const bool isdirty = active && !clean;
        const u64 dw = __ballot(isdirty);
        if ((tid & 63) == 0 && a0 + (tid & ~63) < n) dbits[(size_t)b * ((n + 63) / 64) + (a >> 6)] = dw;
        nd += isdirty;
        if (lst) {
            // the pair kernel's list: dirty curves (bit 31) from the front, clean curves that cross the target from the back
            // (n - 1 entries at most in all); wave-aggregated appends
            const bool wantc = active && clean && (hf & 2);
            const u64 wd = __ballot(isdirty), wc = __ballot(wantc);
            if (wd) {
                u32 base = 0;
                if ((tid & 63) == 0) base = atomicAdd(&lcount, (u32)__popcll(wd));
                base = (u32)__builtin_amdgcn_readfirstlane((int)base);
                if (isdirty) lst[base + (u32)__popcll(wd & ((1ull << (tid & 63)) - 1ull))] = (u32)a | 0x80000000u;
            }
            if (wc) {
                u32 base = 0;
                if ((tid & 63) == 0) base = atomicAdd(&ccount, (u32)__popcll(wc));
                base = (u32)__builtin_amdgcn_readfirstlane((int)base);
                if (wantc) lst[(u32)n - 1u - (base + (u32)__popcll(wc & ((1ull << (tid & 63)) - 1ull)))] = (u32)a;
            }
        }
        if (active && clean) {
            if (!(hf & 2)) {                       // empty canonical mask: below throughout (side 0) / above throughout
                z0 += side == 0;
                z1 += side == 1;
            } else {
                const u32 bit = (u32)(strict_spread(hf) >> 24) & (FB - 1);
                atomicOr(&fbits[side * (FB / 32) + (bit >> 5)], 1u << (bit & 31));
            }
        }
    }
    __syncthreads();
    // How many candidates?  (The table takes 0.6 of its slots per round; see below.)  Not counted when even all n curves
    // would fit at a load of 0.8.
    int cand = 0;
    u64 f01 = 0, f23 = 0;                                                   // bigf: this thread's candidates, bit = iteration (n < 2^17)
    {
        int it = 0;
        for (i64 a0 = 0; a0 < n && must_count; a0 += ST_ML_THREADS, ++it) {
            const i64 a = a0 + tid;
            const u64 hf = a < n ? hb[a] : 0;
            bool c = false;
            if (a < n && a != tg && (hf & 3) == 3) {
                const u32 side = (u32)(hf >> 2) & 1u;
                const u32 bit = (u32)(strict_spread(hf) >> 24) & (FB - 1);
                c = (fbits[(1u - side) * (FB / 32) + (bit >> 5)] >> (bit & 31)) & 1u;
            }
            if (c) { if (it < 64) f01 |= 1ull << it; else f23 |= 1ull << (it - 64); }
            cand += __syncthreads_count(c);
        }
    }
    if (bigf) {                                                             // the filter has served: its area becomes the table
        __syncthreads();
        for (int e = tid; e < 2 * slots; e += ST_ML_THREADS) tabl[e] = 0;
        __syncthreads();
    }
    // More candidates than the table takes (n in the tens of thousands: the filter fills up and lets half of the crossing
    // curves through): the digests are dealt into `rounds` classes by hash bits of their own and the table is filled
    // class by class (a group lies in one class); more than 16 rounds, or a class that still does not fit: flagged.
    int rounds = (int)(((i64)cand * 5 + (i64)slots * 3 - 1) / ((i64)slots * 3));       // load 0.6 per round
    if (rounds < 1) rounds = 1;
    bool overflow = force_overflow || rounds > 16;                               // block-uniform
    // Pass 2: only the curves whose digest was seen on the other side enter the table (digests again from L2).
    for (int rd = 0; rd < rounds && !overflow; ++rd) {
    if (rd > 0) {
        __syncthreads();
        for (int e = tid; e < 2 * slots; e += ST_ML_THREADS) tabl[e] = 0;
        __syncthreads();
    }
    bool stuck = false;
    int it = 0;
    for (i64 a0 = 0; a0 < n; a0 += ST_ML_THREADS, ++it) {
        const i64 a = a0 + tid;
        if (bigf && !(((it < 64 ? f01 >> it : f23 >> (it - 64))) & 1ull)) continue;   // not a candidate: its digest is not even read
        const u64 hf = a < n ? hb[a] : 0;
        if (a < n && a != tg && (hf & 3) == 3) {
            const u32 side = (u32)(hf >> 2) & 1u;
            const u64 h = strict_spread(hf);
            const u32 bit = (u32)(h >> 24) & (ST_ML_SEEN - 1);
            if ((int)((u32)(h >> 53) % (u32)rounds) == rd &&
                (bigf || ((seen[(1u - side) * (ST_ML_SEEN / 32) + (bit >> 5)] >> (bit & 31)) & 1u))) {
                const u32 tag = ((u32)(h >> 40) & 0x1FFFu) | 0x2000u;       // 14 bits, never zero
                const u32 mine = (tag << 18) | (side << 17) | (u32)a;       // a < 2^17
                int slot = (int)(h & (u64)(slots - 1));
                for (int probe = 0; probe < slots; ++probe) {                // load <= 0.8: always ends early
                    u32 cur = __hip_atomic_load(&tabl[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (cur == 0) {
                        cur = atomicCAS(&tabl[slot], 0u, mine);
                        if (cur == 0) break;
                    }
                    if ((cur >> 18) == tag) {
                        const i64 rep = (i64)(cur & 0x1FFFFu);
                        const u64 hr = hb[rep];
                        if (strict_same_canonical(mb, n, W32, lastvalid, cmask, a, hf, rep, hr)) {
                            const u32 rside = (cur >> 17) & 1u;
                            const u32 old = atomicAdd(&cntl[slot], side ? 0x10000u : 1u);
                            acc += side ? (old & 0xFFFFu) + (rside == 0) : (old >> 16) + (rside == 1);
                            // the two side counts share one word: a group with more than 65 535 later members on one
                            // side would carry into the other half -- such a target goes to the global-memory table
                            // (full 32-bit counters), which recounts ALL its groups
                            stuck |= (side ? old >> 16 : old & 0xFFFFu) == 0xFFFFu;
                            break;
                        }
                    }
                    slot = (slot + 1) & (slots - 1);
                    stuck |= probe == slots - 1;                             // table full: never with load 0.6, but exact
                }
            }
        }
    }
    if (__syncthreads_or(stuck)) overflow = true;
    }                                                                         // rounds
    if (overflow) acc = 0;                                                    // the global-memory table counts ALL groups
    u64 r0 = acc, r1 = ((u64)z0 << 32) | z1, r2 = nd;
    for (int o = 32; o > 0; o >>= 1) {
        r0 += __shfl_down(r0, o);
        r1 += __shfl_down(r1, o);
        r2 += __shfl_down(r2, o);
    }
    if ((tid & 63) == 0) { red[tid >> 6][0] = r0; red[tid >> 6][1] = r1; red[tid >> 6][2] = r2; }
    __syncthreads();
    if (tid == 0) {
        u64 t0 = 0, t1 = 0, t2 = 0;
        for (int k = 0; k < ST_ML_THREADS / 64; ++k) { t0 += red[k][0]; t1 += red[k][1]; t2 += red[k][2]; }
        meta[b * 4] = (u32)t2;
        meta[b * 4 + 3] = overflow ? 1u : 0u;                 // the global-table kernels add this target's groups
        if (ilist) {
            u32 *hd = ilist + (size_t)b * (n + 4);
            hd[0] = lcount;                                   // dirty entries lst[0 .. hd[0]); clean ones lst[n - hd[3] .. n)
            hd[3] = ccount;
            hd[1] = (u32)(t1 >> 32);                          // z0: clean curves below the target throughout
            hd[2] = (u32)t1;                                  // z1: ... above it throughout
        }
        if (t2) dlist[atomicAdd(dcount, 1u)] = (u32)b;        // the pair kernel's work list
        // with whole_targets the pair kernel that follows counts ALL pairs of a target that has dirty curves
        if (!(whole_targets && t2)) out[(q0 + b) * jcols] = t0 + (t1 >> 32) * (t1 & 0xFFFFFFFFull);
    }
}

// Targets the LDS kernel flagged (meta[b][3]: more candidates than its table takes): the same grouping in a table in
// global memory (64-bit keys: 47 tag bits | 17-bit id; two counters per slot; >= 2n slots).  The LDS kernel has done
// the rest (dirty curves, empty masks, work list, out = z0 * z1); these kernels add the groups' products.
// grid = (ceil(slots / 4096), nb): zero the flagged targets' tables
__global__ __launch_bounds__(ST_THREADS) void strict_match_clear_kernel(const u32 *__restrict__ meta, unsigned long long *__restrict__ keys,
                                                                       u32 *__restrict__ cnt, i64 slots) {
    const i64 b = blockIdx.y;
    if (!meta[b * 4 + 3]) return;
    const i64 i0 = (i64)blockIdx.x * 4096;
    for (i64 i = i0 + threadIdx.x; i < i0 + 4096 && i < slots; i += ST_THREADS) {
        keys[(size_t)b * slots + i] = 0;
        cnt[((size_t)b * slots + i) * 2] = 0;
        cnt[((size_t)b * slots + i) * 2 + 1] = 0;
    }
}

// grid = (ceil(n / 256), nb)
__global__ __launch_bounds__(ST_THREADS) void strict_match_insert_kernel(
    const u32 *__restrict__ m32, const u64 *__restrict__ HF, i64 T, i64 n, const i64 *__restrict__ targets, i64 q0,
    const u32 *__restrict__ xnan, const u32 *__restrict__ cmask, const u32 *__restrict__ meta,
    unsigned long long *__restrict__ keys, u32 *__restrict__ cnt, i64 slots) {
    const i64 b = blockIdx.y;
    if (xnan[b] || !meta[b * 4 + 3]) return;
    const i64 tg = targets ? targets[q0 + b] : q0 + b;
    const i64 a = (i64)blockIdx.x * ST_THREADS + threadIdx.x;
    if (a >= n || a == tg) return;
    const int W32 = (int)((T + 31) / 32);
    const u32 lastvalid = (T & 31) ? ((1u << (T & 31)) - 1u) : 0xFFFFFFFFu;
    const u32 *mb = m32 + (size_t)b * 2 * W32 * n;
    const u64 hf = HF[(size_t)b * n + a];
    if ((hf & 3) != 3) return;                                // dirty, or the empty canonical mask: counted already
    const u32 side = (u32)(hf >> 2) & 1u;
    const u64 h = strict_spread(hf);
    const u64 tag = (h >> 17) | ((u64)1 << 46);               // 47 bits, never zero
    const unsigned long long mine = (tag << 17) | (u64)a;
    unsigned long long *kb = keys + (size_t)b * slots;
    u32 *cb = cnt + (size_t)b * slots * 2;
    i64 slot = (i64)(h & (u64)(slots - 1));
    for (i64 probe = 0; probe < slots; ++probe) {             // the table has >= 2n slots: always ends early
        unsigned long long cur = __hip_atomic_load(&kb[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(&kb[slot], 0ull, mine);
            if (cur == 0) break;
        }
        if ((cur >> 17) == tag) {
            const i64 rep = (i64)(cur & 0x1FFFF);
            if (strict_same_canonical(mb, n, W32, lastvalid, cmask, a, hf, rep, HF[(size_t)b * n + rep])) break;
        }
        slot = (slot + 1) & (slots - 1);
    }
    atomicAdd(&cb[slot * 2 + side], 1u);
}

// grid = (nb, ceil(slots / ST_TOTAL_CHUNK)): the flagged targets' sums of count(side 0) * count(side 1)
constexpr int ST_TOTAL_CHUNK = 4096;
__global__ __launch_bounds__(ST_THREADS) void strict_match_total_kernel(
    const u32 *__restrict__ cnt, i64 slots, i64 q0, const u32 *__restrict__ xnan, const u32 *__restrict__ meta,
    int whole_targets, u64 *__restrict__ out, int jcols) {
    __shared__ u64 scratch[ST_THREADS / 64];
    const i64 b = blockIdx.x;
    if (xnan[b] || !meta[b * 4 + 3]) return;
    if (whole_targets && meta[b * 4] != 0) return;   // the pair kernel that follows counts ALL pairs of such a target
    const uint2 *cb = reinterpret_cast<const uint2 *>(cnt) + (size_t)b * slots;
    const i64 i0 = (i64)blockIdx.y * ST_TOTAL_CHUNK;
    const i64 i1 = i0 + ST_TOTAL_CHUNK < slots ? i0 + ST_TOTAL_CHUNK : slots;
    u64 acc = 0;
    for (i64 i = i0 + threadIdx.x; i < i1; i += ST_THREADS) {
        const uint2 c = cb[i];
        acc += (u64)c.x * (u64)c.y;
    }
    const u64 tot = block_sum(acc, scratch);
    if (threadIdx.x == 0 && tot) atomicAdd(&out[(q0 + b) * jcols], tot);
}

// J = 3 / 4: one thread per (J-1)-prefix, loop over the last member.
template <int J>
__global__ __launch_bounds__(ST_THREADS) void strict_subsets_kernel(
    const u64 *__restrict__ masks, i64 T, i64 n, const i64 *__restrict__ targets, i64 q0,
    const u32 *__restrict__ xnan, u64 *__restrict__ out, int jcols) {
    __shared__ u64 scratch[ST_THREADS / 64];
    i64 b = blockIdx.z;
    i64 q = q0 + b;
    if (xnan[b]) return;
    i64 tg = targets ? targets[q] : q;
    int W = (int)((T + 63) / 64);
    const u64 *mb = masks + (size_t)b * n * 2 * W;
    // prefix (i0 < i1 [< i2]) from a flat index over n^(J-1)
    i64 flat = (i64)blockIdx.x * ST_THREADS + threadIdx.x;
    i64 idx[3];
    bool ok = true;
    i64 f = flat;
    for (int k = J - 2; k >= 0; --k) { idx[k] = f % n; f /= n; }
    if (f != 0) ok = false;
    for (int k = 0; k < J - 1; ++k) {
        if (idx[k] == tg) ok = false;
        if (k > 0 && idx[k] <= idx[k - 1]) ok = false;
    }
    u64 good = 0;
    if (ok) {
        for (i64 c = idx[J - 2] + 1; c < n; ++c) {
            if (c == tg) continue;
            u64 bad = 0;
            for (int w = 0; w < W; ++w) {
                u64 u = mb[(size_t)c * 2 * W + w], d = mb[(size_t)c * 2 * W + W + w];
                for (int k = 0; k < J - 1; ++k) {
                    u &= mb[(size_t)idx[k] * 2 * W + w];
                    d &= mb[(size_t)idx[k] * 2 * W + W + w];
                }
                bad |= u | d;
            }
            good += (bad == 0);
        }
    }
    u64 tot = block_sum(good, scratch);
    if (threadIdx.x == 0 && tot) atomicAdd(&out[q * jcols + (J - 2)], tot);
}

// ---- host side: which routes a call takes, what workspace they need, and the launches ----
constexpr i64 ST_RANK_MAXN = 32767;  // ranks below 2^15 (two per register in the mask kernel); images: bucket kernel up to 16 384 curves, its column-block form beyond
// 32 767 < n <= 131 071: 32-bit ranks from the large-n route's B image (strict_masks_rank32_kernel)
static inline bool strict_rank32_applies(i64 T, i64 n, int J) { return J == 2 && n > ST_RANK_MAXN && n <= 131071 && mbd_rank_big_supported(T, n, 2); }
static inline i64 strict_words(i64 T) { return (T + 63) / 64; }
static inline i64 strict_words32(i64 T) { return (T + 31) / 32; }
// complement matching: the global-memory table behind the LDS one (strict_match_insert_kernel): slot = 64-bit key + two counters
static inline i64 strict_table_slots(i64 n) { i64 s = 64; while (s < 2 * n) s <<= 1; return s; }

// The route plan: the only place of the strict path that reads a cross-check switch.
StrictPlan strict_plan(i64 T, i64 n, i64 m, int J, bool external) {
    const bool v1 = xswitch("SD_STRICT_V1") == 1;                          // the first-generation kernels only
    const bool noclass = v1 || xswitch("SD_STRICT_NOCLASS") == 1;          // short series through the mask kernels like any other
    const bool fp64 = v1 || xswitch("SD_STRICT_FP64_MASKS") == 1;          // masks from the fp64 values at any n
    StrictPlan p;
    p.classes = !noclass && strict_class_applies(T, n, J);
    // all targets, or a subset that is not small (else the state-class kernel's O(m n) is less work)
    p.grid = !noclass && !external && bd_strict_grid_applies(T, n, J) && m * 32 >= n && xswitch("SD_STRICT_NOGRID") != 1;
    p.laneclass = xswitch("SD_STRICT_LANECLASS") == 1;
    p.class_wg = !noclass && strict_class_wg_applies(T, J);
    p.class_wg_only = strict_class_wg_only(T, n, m, J);
    p.match = !v1 && strict_match_applies(T, n, J) && xswitch("SD_STRICT_NOMATCH") != 1;
    p.rankmasks = !fp64 && !external && n >= 2 && n <= ST_RANK_MAXN && J == 2;
    p.rank32 = !fp64 && !external && strict_rank32_applies(T, n, J);
    p.gen2 = !v1 && J == 2 && strict_words32(T) <= ST_W32;
    p.force_global = xswitch("SD_STRICT_GLOBAL_TABLE") == 1;
    p.pairs2 = xswitch("SD_STRICT_PAIRS2") == 1;
    return p;
}

// The workspace of the mask pipeline for batches of b targets: every buffer, its size and its place, stated once.  The size
// functions read `total` (null base); the launcher gives the base and uses the pointers.  plan.rankmasks / plan.rank32 say
// which rank image is laid out; nothing else of the plan changes the layout.
struct StrictWs {
    i64 b, slots;                        // targets per batch; slots of a target's global-memory table
    u64 *masks;                          // first generation: u64 [b][n][2 W]; second: the u32 word-major image over the same bytes
    u32 *xnan, *cmask;                   // [b] NaN in the target; timepoints that do not count
    unsigned long long *keys;            // global-memory table: keys [b][slots] | counters [b][slots][2] | per target
    u32 *cnt, *dirty; u64 *dbits;        //   {dirty, below, above, overflow} | dirty bitmaps [b][ceil(n / 64)]
    double *Yt; u64 *HF;                 // the batch's targets, gathered (values or ranks); hash + flags per (target, curve)
    unsigned char *dflag;                // dirty (target, curve) pairs
    u32 *dlist, *dcount, *ilist;         // dirty targets of the batch | their number; per target the pair kernel's list of curves
    u32 *R, *rnan, *tiemask;             // rank image [T][n], NaN counts per row, timepoints with ties (rank masks only)
    void *bigws;                         // the large-n route's scratch for its image (32-bit ranks only)
    size_t bigws_bytes, total;
};
static StrictWs strict_layout(const StrictPlan &plan, i64 T, i64 n, i64 b, void *base) {
    StrictWs w{};
    size_t o = 0;                        // (integer arithmetic: the size functions lay out from a null base)
    auto take = [&](size_t bytes) { const uintptr_t p = (uintptr_t)base + o; o += align_up(bytes, 256); return p; };
    const i64 W32 = strict_words32(T), dwords = (n + 63) / 64;
    w.b = b, w.slots = strict_table_slots(n);
    w.masks = (u64 *)take((size_t)b * n * 2 * strict_words(T) * 8);
    w.xnan = (u32 *)take((size_t)b * 4);
    const uintptr_t tab = take((size_t)b * (w.slots * 16 + 16 + dwords * 8));
    w.keys = (unsigned long long *)tab;
    w.cnt = (u32 *)(tab + (size_t)b * w.slots * 8);
    w.dirty = (u32 *)(tab + (size_t)b * w.slots * 16);
    w.dbits = (u64 *)(tab + (size_t)b * (w.slots * 16 + 16));
    w.cmask = (u32 *)take((size_t)W32 * 4);
    w.Yt = (double *)take((size_t)b * W32 * 256);
    w.HF = (u64 *)take((size_t)b * n * 8);
    w.dflag = (unsigned char *)take((size_t)b * n);
    w.dlist = (u32 *)take((size_t)(b + 1) * 4);
    w.dcount = (u32 *)((uintptr_t)w.dlist + (size_t)b * 4);
    w.ilist = (u32 *)take((size_t)b * (n + 4) * 4);
    if (plan.rankmasks || plan.rank32) {
        w.R = (u32 *)take((size_t)T * n * 4);
        w.rnan = (u32 *)take((size_t)T * 4);
        w.tiemask = (u32 *)take((size_t)T * 4);              // W32 words are used; T words have always been reserved
    }
    if (plan.rank32) w.bigws = (void *)take(w.bigws_bytes = mbd_rank_big_workspace_bytes(T, n, 2));
    w.total = o + 2560;                                      // ten buffers' worth of alignment slack, reserved since the first layout
    return w;
}
// What the size functions report: the layout of the most demanding plan of the shape -- the rank image whenever n allows it,
// whatever J, the targets and the switches -- so the launcher's own layout never takes more than was asked for.
static size_t strict_ws_for_batch(i64 T, i64 n, i64 b) {
    StrictPlan most{};
    most.rankmasks = n <= ST_RANK_MAXN;
    most.rank32 = strict_rank32_applies(T, n, 2);
    return strict_layout(most, T, n, b, nullptr).total;
}
// The recommended batch: up to 2 GiB of masks and tables.  `per` approximates what one more target adds to strict_layout (the
// b-proportional buffers without their alignment); a closed formula because the batch sizes it gives are what callers see.
static i64 strict_batch(i64 T, i64 n, i64 m) {
    size_t per = (size_t)n * 2 * strict_words(T) * 8 + (size_t)strict_table_slots(n) * 16 + 20 + (size_t)((n + 63) / 64) * 8 + (size_t)strict_words32(T) * 256 + (size_t)n * 13 + 16;
    i64 b = (i64)(((size_t)2048 << 20) / (per ? per : 1));
    if (b < 1024) {                                           // ... or 16 GiB when that is what 1024 targets take: the matching
        const i64 b16 = (i64)(((size_t)16384 << 20) / (per ? per : 1));   // kernel runs one workgroup per target
        b = b16 < 1024 ? b16 : 1024;
    }
    if (b < 1) b = 1;
    if (b > m) b = m;
    return b > 65535 ? 65535 : b;
}
// largest batch (<= the recommended one) whose layout fits ws_bytes; 0: not even one target fits
static i64 strict_batch_for_ws(i64 T, i64 n, i64 m, size_t ws_bytes) {
    i64 hi = strict_batch(T, n, m);
    if (strict_ws_for_batch(T, n, hi) <= ws_bytes) return hi;
    if (strict_ws_for_batch(T, n, 1) > ws_bytes) return 0;
    i64 lo = 1;                                               // fits
    while (hi - lo > 1) {
        const i64 mid = lo + (hi - lo) / 2;
        if (strict_ws_for_batch(T, n, mid) <= ws_bytes) lo = mid; else hi = mid;
    }
    return lo;
}

// The RECOMMENDED size (batches of strict_batch targets).  The launchers take any workspace that holds a batch of one target and
// size their batches to what they are given (strict_batch_for_ws): bd_strict_min_workspace_bytes is the floor.
size_t bd_strict_workspace_bytes(i64 T, i64 n, i64 m, int J) {
    const StrictPlan p = strict_plan(T, n, m, J, false);
    // short series go through the class kernels: a flag, no images -- or through the grid of cells (rank image, records in
    // three orders, cell histogram, class counts)
    if (p.grid) return bd_strict_grid_workspace_bytes(T, n, m < n) + 4096;
    if (p.classes || p.class_wg_only) return 4096;
    // 6 ... 8 timepoints: the class kernel's flag in front of what the mask pipeline takes should the data hold NaN
    return strict_ws_for_batch(T, n, strict_batch(T, n, m)) + (strict_class_wg_applies(T, J) ? 256 : 0);
}
// what a caller who KNOWS the data NaN-free needs: the flag alone where the state classes of 6 ... 8 timepoints take such data
size_t bd_strict_nanfree_workspace_bytes(i64 T, i64 n, i64 m, int J) {
    return strict_plan(T, n, m, J, false).class_wg ? (size_t)4096 : bd_strict_workspace_bytes(T, n, m, J);
}
size_t bd_strict_min_workspace_bytes(i64 T, i64 n, i64 m, int J) {
    const StrictPlan p = strict_plan(T, n, m, J, false);
    if (p.classes || p.class_wg_only) return 4096;
    return strict_ws_for_batch(T, n, 1) + (strict_class_wg_applies(T, J) ? 256 : 0);
}
// what launch_bd_strict needs to be called at all: 6 ... 8 timepoints get by with the flag when the data is NaN-free, which the
// launcher finds out itself; data with NaN then meets the mask pipeline's own check of what it was given
size_t bd_strict_launch_floor_bytes(i64 T, i64 n, i64 m, int J) {
    return strict_class_wg_applies(T, J) ? (size_t)256 : bd_strict_min_workspace_bytes(T, n, m, J);
}
size_t bd_strict_external_workspace_bytes(i64 T, i64 n, i64 m) { return bd_strict_workspace_bytes(T, n, m, 2) + align_up((size_t)m * 8, 256); }

// One call of the mask pipeline: its arguments, plan and buffers.  Every stage is a fixed sequence of launches on s; run()
// strings them together per batch of nb targets from q0.
struct StrictRun {
    const double *Y, *Q;         // Q non-null: the m targets are EXTERNAL curves (T x m, time-major); every curve of Y is an "other"
    const i64 *targets;
    i64 T, n, m;
    int J, jcols;                // jcols = J - 1 columns of out per target
    u64 *out;
    hipStream_t s;
    StrictPlan p;
    StrictWs w;                  // laid out for batches of w.b targets
    const u32 *m32() const { return (const u32 *)w.masks; }   // the second generation's view of the mask buffer
    dim3 curves(i64 nb) const { return dim3((unsigned)((n + ST_THREADS - 1) / ST_THREADS), (unsigned)nb); }
    dim3 pairs(i64 nb) const { return dim3((unsigned)((n + ST_THREADS - 1) / ST_THREADS), (unsigned)((n + ST_BCHUNK - 1) / ST_BCHUNK), (unsigned)nb); }
    int rank_images() const;
    void gather_targets(i64 q0, i64 nb) const;
    void masks_gen2(i64 q0, i64 nb, const StrictMaskOut &mo) const;
    int matching(i64 q0, i64 nb) const;
    void pairs_gen2(i64 q0, i64 nb, bool matched) const;
    void first_generation(i64 q0, i64 nb, const u32 *gate, bool gathered) const;
    int run() const;
};

// The integer rank image the mask kernels compare instead of the values, and the timepoints at which any two curves tie
int StrictRun::rank_images() const {
    if (!p.rankmasks && !p.rank32) return SD_OK;
    if (int rc = p.rank32 ? launch_rank_big_image(Y, T, n, w.R, w.rnan, w.bigws, w.bigws_bytes, s) : SD_OK) return rc;
    const i64 step = 2048 * 64;                               // the 16-bit image launchers take at most 2048 rows per workgroup
    for (i64 r0 = 0; p.rankmasks && r0 < T; r0 += step) {
        const i64 rows = T - r0 < step ? T - r0 : step;
        if (int rc = n <= 16384 ? launch_rank_bucket_image(Y, n, r0, rows, w.R + r0 * n, w.rnan + r0, s)
                                : launch_rank_medium_image(Y, n, r0, rows, w.R + r0 * n, w.rnan + r0, s)) return rc;
    }
    SD_HIP(hipMemsetAsync(w.tiemask, 0, (size_t)strict_words32(T) * 4, s));
    if (p.rankmasks)
        hipLaunchKernelGGL(strict_row_ties_kernel, dim3((unsigned)T), dim3(ST_THREADS), 0, s, (const u32 *)w.R, (const u32 *)w.rnan, n, w.tiemask);
    else
        hipLaunchKernelGGL(strict_row_ties32_kernel, dim3((unsigned)T), dim3(ST_THREADS), 0, s, (const u32 *)w.R, n, w.tiemask);
    return SD_OK;
}

// The batch's targets gathered into Yt -- ranks or values, as the plan's mask kernel reads them; xnan notes a NaN target
void StrictRun::gather_targets(i64 q0, i64 nb) const {
    const dim3 g((unsigned)nb), t(ST_THREADS);
    if (p.rankmasks)
        hipLaunchKernelGGL(strict_gather_rank_targets_kernel, g, t, 0, s, (const u32 *)w.R, T, n, targets, q0, (u32 *)w.Yt, w.xnan);
    else if (p.rank32)
        hipLaunchKernelGGL(strict_gather_rank32_targets_kernel, g, t, 0, s, (const u32 *)w.R, T, n, targets, q0, (u32 *)w.Yt, w.xnan);
    else
        hipLaunchKernelGGL(strict_gather_targets_kernel, g, t, 0, s, Y, T, n, targets, q0, Q, m, w.Yt, w.xnan);
}
// Second-generation masks (32-bit words, word-major image over the bytes of w.masks: 2 W32 n u32 <= 2 W n u64) as `mo` asks.
// The pass over every target of the batch (no list) gathers the targets first; the pass over the listed ones reuses them.
void StrictRun::masks_gen2(i64 q0, i64 nb, const StrictMaskOut &mo) const {
    const dim3 g((unsigned)((n + ST_THREADS - 1) / ST_THREADS), (unsigned)strict_words32(T), (unsigned)((nb + ST_TG - 1) / ST_TG)), t(ST_THREADS);
    if (!mo.dlist) gather_targets(q0, nb);
    if (p.rankmasks)
        hipLaunchKernelGGL(strict_masks_rank_kernel, g, t, 0, s, (const u32 *)w.R, (const u32 *)w.Yt, T, n, nb, mo);
    else if (p.rank32)
        hipLaunchKernelGGL(strict_masks_rank32_kernel, g, t, 0, s, (const u32 *)w.R, (const u32 *)w.Yt, T, n, nb, mo);
    else
        hipLaunchKernelGGL(strict_masks2_kernel, g, t, 0, s, Y, (const double *)w.Yt, T, n, nb, mo);
}

// Complement matching over the UN masks of the batch: digests, the LDS table per target, and behind it the global-memory table for
// the targets the LDS kernel flags.  Leaves the clean-clean counts in out, the dirty curves per target in w.dirty / w.dbits / w.ilist
// and the targets that have any in w.dlist.
int StrictRun::matching(i64 q0, i64 nb) const {
    const dim3 t(ST_THREADS);
    const int whole_targets = p.gen2 ? 0 : 1;                 // T > 1024: the first generation counts ALL pairs of a dirty target
    hipLaunchKernelGGL(strict_hash_kernel, curves(nb), t, 0, s, m32(), T, n, w.xnan, (const u32 *)w.cmask, (const unsigned char *)w.dflag, w.HF);
    SD_HIP(hipMemsetAsync(w.dirty, 0, (size_t)w.b * 16, s));
    SD_HIP(hipMemsetAsync(w.dcount, 0, 4, s));
    const i64 lslots = strict_lds_slots(n);
    const size_t tb = (size_t)lslots * 8 + 2 * (ST_ML_SEEN / 8);
    SD_HIP(hipFuncSetAttribute((const void *)strict_match_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tb));
    hipLaunchKernelGGL(strict_match_lds_kernel, dim3((unsigned)nb), dim3(ST_ML_THREADS), tb, s, m32(), (const u64 *)w.HF, T, n, targets, q0,
                       w.xnan, (const u32 *)w.cmask, w.dirty, w.dbits, w.dlist, w.dcount, (int)lslots, whole_targets, p.force_global ? 1 : 0,
                       out, jcols, (p.gen2 && !p.pairs2) ? w.ilist : (u32 *)nullptr);
    if (p.force_global || n > ST_MATCH_LDS_CAP) {
        hipLaunchKernelGGL(strict_match_clear_kernel, dim3((unsigned)((w.slots + 4095) / 4096), (unsigned)nb), t, 0, s, (const u32 *)w.dirty,
                           w.keys, w.cnt, w.slots);
        hipLaunchKernelGGL(strict_match_insert_kernel, curves(nb), t, 0, s, m32(), (const u64 *)w.HF, T, n, targets, q0, w.xnan,
                           (const u32 *)w.cmask, (const u32 *)w.dirty, w.keys, w.cnt, w.slots);
        hipLaunchKernelGGL(strict_match_total_kernel, dim3((unsigned)nb, (unsigned)((w.slots + ST_TOTAL_CHUNK - 1) / ST_TOTAL_CHUNK)), t, 0, s,
                           (const u32 *)w.cnt, w.slots, q0, w.xnan, (const u32 *)w.dirty, whole_targets, out, jcols);
    }
    return SD_OK;
}

// Second generation, the pairs the matching has not counted: with matching the pairs with a dirty curve of the targets on
// the work list, without it every pair of every target
void StrictRun::pairs_gen2(i64 q0, i64 nb, bool matched) const {
    const dim3 g2 = pairs(nb), t(ST_THREADS);
    if (!matched) {
        hipLaunchKernelGGL(strict_pairs2_kernel, g2, t, 0, s, m32(), T, n, targets, q0, w.xnan, (const u32 *)nullptr, (const u32 *)nullptr,
                           (const u64 *)nullptr, out, jcols);
    } else if (p.pairs2) {
        // about 8 192 blocks in all (32 layers at least while a layer is small): with no dirty target every block only reads
        // the list's length and leaves
        const i64 per_layer = (i64)g2.x * g2.y;
        i64 layers = (8192 + per_layer - 1) / per_layer;
        if (layers < ST_PAIR_LAYERS && per_layer <= 256) layers = ST_PAIR_LAYERS;
        if (layers > nb) layers = nb;
        hipLaunchKernelGGL(strict_pairs2_kernel, dim3(g2.x, g2.y, (unsigned)layers), t, 0, s, m32(), T, n, targets, q0, w.xnan,
                           (const u32 *)w.dlist, (const u32 *)w.dcount, (const u64 *)w.dbits, out, jcols);
    } else {
        const int tiles = (int)((n + ST_P3_THREADS - 1) / ST_P3_THREADS);
        const int chunks = n > 4096 ? 8 : (n > 1024 ? 4 : 1);
        const i64 items = (i64)nb * tiles * chunks, grid = items > 1024 ? 1024 : items;
        hipLaunchKernelGGL(strict_pairs3_kernel, dim3((unsigned)grid), dim3(ST_P3_THREADS), 0, s, m32(), T, n, q0, (const u32 *)w.dlist,
                           (const u32 *)w.dcount, (const u32 *)w.ilist, out, jcols, tiles, chunks);
    }
}

// First generation: u64 masks in its own layout (over the image the second generation has consumed: stream order), every pair
// tested, prefixes enumerated for J = 3, 4.  gate: the matching's per-target dirty counts (null: every target) -- past 1 024
// timepoints the second generation's pair kernel does not apply.  gathered: Yt holds the external targets' values already.
void StrictRun::first_generation(i64 q0, i64 nb, const u32 *gate, bool gathered) const {
    const dim3 g2 = pairs(nb), t(ST_THREADS);
    if (Q && !gathered) gather_targets(q0, nb);             // external targets reach the first generation through their gathered copy
    hipLaunchKernelGGL(strict_masks_kernel, curves(nb), t, 0, s, Y, T, n, targets, q0, w.masks, w.xnan, gate,
                       Q ? (const double *)w.Yt : (const double *)nullptr);
    if (strict_words(T) <= ST_WREG)
        hipLaunchKernelGGL((strict_pairs_kernel<true>), g2, t, 0, s, w.masks, T, n, targets, q0, w.xnan, gate, out, jcols);
    else
        hipLaunchKernelGGL((strict_pairs_kernel<false>), g2, t, 0, s, w.masks, T, n, targets, q0, w.xnan, gate, out, jcols);
    if (J >= 3) {
        const dim3 g3((unsigned)((n * n + ST_THREADS - 1) / ST_THREADS), 1, (unsigned)nb);
        hipLaunchKernelGGL((strict_subsets_kernel<3>), g3, t, 0, s, w.masks, T, n, targets, q0, w.xnan, out, jcols);
    }
    if (J >= 4) {
        const dim3 g4((unsigned)((n * n * n + ST_THREADS - 1) / ST_THREADS), 1, (unsigned)nb);
        hipLaunchKernelGGL((strict_subsets_kernel<4>), g4, t, 0, s, w.masks, T, n, targets, q0, w.xnan, out, jcols);
    }
}

// The whole pipeline in batches of w.b targets
int StrictRun::run() const {
    const i64 B = w.b;
    SD_HIP(hipMemsetAsync(out, 0, sizeof(u64) * m * jcols, s));
    if (J >= 3 && (double)n * (double)n * (J >= 4 ? (double)n : 1.0) > 4.0e9)      // one thread per (J-1)-prefix
        return fail(SD_ERR_UNSUPPORTED, "strict J=%d enumeration too large for n=%lld", J, (long long)n);
    if (p.match) {
        SD_HIP(hipMemsetAsync(w.cmask, 0, (size_t)strict_words32(T) * 4, s));
        // (an external target does not share a value all of Y's curves share: every timepoint counts for it)
        if (!Q) hipLaunchKernelGGL(strict_const_rows_kernel, dim3((unsigned)T), dim3(ST_THREADS), 0, s, Y, T, n, w.cmask);
    }
    if (int rc = rank_images()) return rc;
    for (i64 q0 = 0; q0 < m; q0 += B) {
        const i64 nb = m - q0 < B ? m - q0 : B;
        SD_HIP(hipMemsetAsync(w.xnan, 0, (size_t)nb * 4, s));
        const u32 *gate = nullptr;
        if (p.gen2 || p.match) {
            // with matching, the first pass stores UN words and dirty flags only (see StrictMaskOut)
            if (p.match) SD_HIP(hipMemsetAsync(w.dflag, 0, (size_t)nb * n, s));
            masks_gen2(q0, nb, StrictMaskOut{(u32 *)w.masks, p.match ? w.dflag : nullptr, w.cmask, w.tiemask, nullptr, nullptr});
            if (p.match) {
                if (int rc = matching(q0, nb)) return rc;
                gate = w.dirty;
                // second pass: full masks (UN and DN) for the targets on the pair kernel's work list
                if (p.gen2) masks_gen2(q0, nb, StrictMaskOut{(u32 *)w.masks, nullptr, w.cmask, w.tiemask, w.dlist, w.dcount});
            }
        }
        if (p.gen2) pairs_gen2(q0, nb, gate != nullptr);
        else first_generation(q0, nb, gate, p.match);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

static int launch_bd_strict_impl(const double *Y, i64 T, i64 n, const i64 *targets, const double *Q, i64 m, int J, u64 *out, void *ws, size_t ws_bytes, hipStream_t s) {
    StrictRun r{Y, Q, targets, T, n, m, J, J - 1, out, s, strict_plan(T, n, m, J, Q != nullptr), StrictWs{}};
    if (r.p.classes) return launch_bd_strict_classes(r.p, Y, T, n, Q ? nullptr : targets, Q, m, out, 1, ws, ws_bytes, s);
    // 6 ... 8 timepoints: the workgroup form of the class kernel when no value is NaN.  That is a property of the data: the flag comes
    // back to the host (one 4-byte copy and a wait: the only route that waits); data with NaN goes on behind the 256-byte flag
    if (r.p.class_wg && m > 0 && n > 0) {
        if (!ws || ws_bytes < 256) return fail(SD_ERR_WORKSPACE, "strict-depth workspace too small");
        u32 *flag = (u32 *)ws, hflag = 0;
        SD_HIP(hipMemsetAsync(flag, 0, 4, s));
        launch_strict_any_nan(Y, T, n, Q, m, flag, s);
        SD_HIP(hipMemcpyAsync(&hflag, flag, 4, hipMemcpyDeviceToHost, s));
        SD_HIP(hipStreamSynchronize(s));
        if (!hflag) return launch_bd_strict_class_wg(Y, T, n, Q ? nullptr : targets, Q, m, nullptr, out, 1, s);
        if (r.p.class_wg_only)
            return fail(SD_ERR_UNSUPPORTED, "strict band depth of %lld curves over %lld timepoints with NaN in the data: the state "
                        "classes of 6 to 8 timepoints take NaN-free data, matching takes up to %lld curves", (long long)n,
                        (long long)T, (long long)ST_MATCH_MAXN);
        ws = (char *)ws + 256;
        ws_bytes -= 256;
    }
    const i64 B = strict_batch_for_ws(T, n, m, ws_bytes);     // the recommended batch, or what the caller's workspace holds
    if (B < 1) return fail(SD_ERR_WORKSPACE, "strict-depth workspace too small: %zu bytes, one target takes %zu "
                           "(sd_bd_strict_min_workspace_bytes)", ws_bytes, strict_ws_for_batch(T, n, 1));
    if (!r.p.match && J == 2 && strict_pair_tests_refused(n, m))
        return fail(SD_ERR_UNSUPPORTED, "strict band depth of %lld curves over %lld timepoints: pairs are counted by matching for up to "
                    "%lld curves (any number for T <= 5, and for T <= 8 without NaN); beyond that every pair is tested, %.1e tests here", (long long)n,
                    (long long)T, (long long)ST_MATCH_MAXN, strict_pair_tests(n, m));
    r.w = strict_layout(r.p, T, n, B, ws);                    // within what strict_batch_for_ws measured for B
    if (!ws || r.w.total > ws_bytes) return fail(SD_ERR_WORKSPACE, "strict-depth workspace too small");
    return r.run();
}

int launch_bd_strict(const double *Y, i64 T, i64 n, const i64 *targets, i64 m, int J, u64 *out, void *ws, size_t ws_bytes, hipStream_t s) {
    return launch_bd_strict_impl(Y, T, n, targets, nullptr, m, J, out, ws, ws_bytes, s);
}

int launch_bd_strict_external(const double *Y, i64 T, i64 n, const double *Q, i64 m, u64 *out, void *ws, size_t ws_bytes, hipStream_t s) {
    // the kernels exclude "the target itself" from the others by its column index: -1 for every external target
    Carver cv(ws, ws_bytes);
    i64 *none = (i64 *)cv.take((size_t)m * 8);
    const size_t need = cv.rest();                            // everything behind the index block: the batches adapt to it
    void *sws = cv.take(need);
    if (!none || !sws) return fail(SD_ERR_WORKSPACE, "strict-depth workspace too small (sd_bd_strict_external_workspace_bytes)");
    SD_HIP(hipMemsetAsync(none, 0xFF, (size_t)m * 8, s));
    return launch_bd_strict_impl(Y, T, n, none, Q, m, 2, out, sws, need, s);
}

}  // namespace sd
