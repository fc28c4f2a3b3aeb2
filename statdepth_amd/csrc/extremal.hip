// extremal.hip -- K15: the extremal depth of curves (Narisetty & Nair, JASA 2016).
//
// Definition.  n curves at T timepoints, time-major Y[t][i], no NaN.  For curve q at timepoint t, over the other n - 1
// curves: A = #{strictly above}, B = #{strictly below} (ties in neither: K14's pair).  The pointwise extremity is
//   e_q(t) = |A - B|  in [0, n - 1]          (the paper's pointwise depth is 1 - e / n),
// v_q is the T values e_q(.) sorted in descending order, and curve f is more extreme than or equal to g iff
// v_f >= v_g lexicographically: the paper's comparison of the depth CDFs from the lowest depth level upward, where the
// larger CDF at the first difference is the more extreme curve.  The result per target is
//   G_q = #{ i in the sample : v_i >=lex v_q }      (q itself and every curve with the same vector are counted),
// and the host forms ED = G / n: 1 for the deepest curve, the same depth for identical vectors.
//
// Four stages, every launch bounded in work, no waits between workgroups:
//   1  the pair image of a batch of rows, by K14's two routes (launch_rank_pair_images, rank_depths.hip);
//   2  ex_transform_kernel: E[i][row0 + r] = |A - B| of the batch's rows for ALL n curves, u32, curve-major.  A 64 x 64
//      tile goes through LDS padded to 65 words a row, so the image is read along its rows and E written along its
//      own; partial tiles in both directions are masked;
//   3  ex_sort_kernel: every curve's T values sorted descending in LDS (bitonic network over the next power of two,
//      padded with 0, the smallest value, which sorts last; two strides behind each barrier, four keys a thread), in
//      place in E.  One wave per curve up to 256 padded keys
//      (four curves a workgroup), one workgroup per curve above, up to EX_MAX_T = 16 384 keys = 64 KiB.  The curve's
//      head H[i] is packed on the way out: the first P = min(T, 64 / b) entries in fields of b bits, most significant
//      first, missing fields 0, b = max(16, bit width of n - 1): P = 4 up to 65 536 curves, 3 up to 2^21, 2 beyond.
//      Fields of one width make the order of the u64 the lexicographic order of the prefix;
//   4  ex_rank_kernel: a thread per target, the heads of the sample staged through LDS in tiles of 1024; H_i >= H_q
//      is counted 64 heads at a time, and a group in which some lane met H_i == H_q is gone through again: such a pair
//      walks E[i][P .. T) against E[q][P .. T) to the first difference and is taken off if it is smaller there --
//      a tail of up to 32 entries by the lane alone, a longer one by the wave, which takes the open pairs of its lanes
//      one after the other, 64 entries of both rows at a time.
//      The sample range is split over grid.y so that few targets still fill the machine; the parts meet in integer
//      atomic adds on the zeroed result, which are exact in any order.
#include "curve_routes.h"

namespace sd {

constexpr int EX_TILE = 64;                                        // transpose tile (rows and curves)
constexpr int EX_TILE_WAVES = 8;                                   // its workgroup: 64 x 8 threads
constexpr int EX_WAVE_KEYS = 256;                                  // padded keys one wave sorts; above: one workgroup
constexpr int EX_RANK_THREADS = 256;
constexpr int EX_RANK_TILE = 1024;                                 // heads staged in LDS at a time
constexpr int EX_RANK_SPLIT = 256;                                 // the sample range is split over grid.y in units of this
constexpr int EX_RANK_GROUP = 64;                                  // heads counted in one pass before ties are looked at
constexpr int EX_LANE_WALK = 32;                                   // tail entries a lane walks alone; above: the wave together

template <typename IMG> __device__ __forceinline__ u32 ex_extremity(IMG w);
template <> __device__ __forceinline__ u32 ex_extremity<u32>(u32 w) {
    const u32 A = w >> 16, B = w & 0xFFFFu;
    return A > B ? A - B : B - A;
}
template <> __device__ __forceinline__ u32 ex_extremity<u64>(u64 w) {
    const u32 A = (u32)(w >> 32), B = (u32)w;
    return A > B ? A - B : B - A;
}

// img[rows][n] -> E[i][row0 + r] = |A - B|, E curve-major with rows of T
template <typename IMG>
__global__ __launch_bounds__(EX_TILE * EX_TILE_WAVES) void ex_transform_kernel(const IMG *__restrict__ img, i64 rows, i64 n,
                                                                               i64 row0, i64 T, u32 *__restrict__ E) {
    __shared__ u32 tile[EX_TILE][EX_TILE + 1];
    const int x = threadIdx.x, y = threadIdx.y;
    const i64 c0 = (i64)blockIdx.x * EX_TILE, r0 = (i64)blockIdx.y * EX_TILE;
    for (int k = y; k < EX_TILE; k += EX_TILE_WAVES) {
        const i64 r = r0 + k, c = c0 + x;
        if (r < rows && c < n) tile[k][x] = ex_extremity<IMG>(img[r * n + c]);
    }
    __syncthreads();
    for (int k = y; k < EX_TILE; k += EX_TILE_WAVES) {
        const i64 c = c0 + k, r = r0 + x;
        if (c < n && r < rows) E[c * T + row0 + r] = tile[x][k];
    }
}

template <typename IMG>
static int launch_ex_transform(const IMG *img, i64 row0, i64 rows, i64 n, i64 T, u32 *E, hipStream_t s) {
    const dim3 grid((unsigned)((n + EX_TILE - 1) / EX_TILE), (unsigned)((rows + EX_TILE - 1) / EX_TILE));
    hipLaunchKernelGGL((ex_transform_kernel<IMG>), grid, dim3(EX_TILE, EX_TILE_WAVES), 0, s, img, rows, n, row0, T, E);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

__device__ __forceinline__ void ex_order(u32 &a, u32 &c, bool descending) {
    const u32 lo = a < c ? a : c, hi = a < c ? c : a;
    a = descending ? hi : lo;
    c = descending ? lo : hi;
}

// Rows of E sorted descending in place, H[i] = the packed head.  tpc threads per curve, blockDim.x / tpc curves per
// workgroup, Tp (a power of two, >= 2 and >= T) keys of LDS per curve.  Every thread of the workgroup meets every
// barrier: all curves have the same Tp, and a slot past the last curve sorts zeros.
__global__ __launch_bounds__(1024) void ex_sort_kernel(u32 *__restrict__ E, i64 T, i64 n, int Tp, int tpc, int b, int P,
                                                       u64 *__restrict__ H) {
    extern __shared__ u32 ex_keys[];
    const int slot = threadIdx.x / tpc, lane = threadIdx.x % tpc;
    const i64 q = (i64)blockIdx.x * (blockDim.x / tpc) + slot;
    const bool live = q < n;
    u32 *keys = ex_keys + (size_t)slot * Tp;
    u32 *row = E + (live ? q : 0) * T;
    for (int t = lane; t < Tp; t += tpc) keys[t] = (live && t < T) ? row[t] : 0u;
    __syncthreads();
    for (int k = 2; k <= Tp; k <<= 1) {
        int j = k >> 1;
        for (; j >= 2; j >>= 2) {                                   // strides j and j / 2 behind one barrier: four keys a thread
            const int h = j >> 1;
            for (int idx = lane; idx < (Tp >> 2); idx += tpc) {
                const int lo = idx & (h - 1), i = ((idx - lo) << 2) | lo;      // bits h and j of i are 0
                const bool descending = (i & k) == 0;               // j < k: the same for the four
                u32 k0 = keys[i], k1 = keys[i + h], k2 = keys[i + j], k3 = keys[i + j + h];
                ex_order(k0, k2, descending);
                ex_order(k1, k3, descending);
                ex_order(k0, k1, descending);
                ex_order(k2, k3, descending);
                keys[i] = k0;
                keys[i + h] = k1;
                keys[i + j] = k2;
                keys[i + j + h] = k3;
            }
            __syncthreads();
        }
        if (j == 1) {                                               // an odd number of strides: the last one alone
            for (int idx = lane; idx < (Tp >> 1); idx += tpc) {
                const int i = idx << 1;
                u32 k0 = keys[i], k1 = keys[i + 1];
                ex_order(k0, k1, (i & k) == 0);                     // the last merge (k == Tp) is descending throughout
                keys[i] = k0;
                keys[i + 1] = k1;
            }
            __syncthreads();
        }
    }
    if (!live) return;
    for (int t = lane; t < T; t += tpc) row[t] = keys[t];
    if (lane == 0) {
        u64 h = 0;
        for (int f = 0; f < P; ++f) h = (h << b) | (u64)keys[f];    // P <= T: every field is an entry
        const int fields = 64 / b;
        for (int f = P; f < fields; ++f) h <<= b;                   // missing fields 0
        H[q] = h;
    }
}

// out[q] += #{ i in [s0, s1) : v_i >=lex v_target(q) }, [s0, s1) the blockIdx.y-th chunk of the sample
__global__ __launch_bounds__(EX_RANK_THREADS) void ex_rank_kernel(const u64 *__restrict__ H, const u32 *__restrict__ E, i64 T,
                                                                  i64 n, int P, const i64 *__restrict__ targets, i64 m,
                                                                  i64 chunk, unsigned long long *__restrict__ out) {
    __shared__ u64 heads[EX_RANK_TILE];
    const i64 q = (i64)blockIdx.x * EX_RANK_THREADS + threadIdx.x;
    const bool live = q < m;
    const i64 iq = live ? (targets ? targets[q] : q) : 0;
    const u64 hq = H[iq];
    const int lane = threadIdx.x & 63;
    const i64 s0 = (i64)blockIdx.y * chunk, s1 = s0 + chunk < n ? s0 + chunk : n;
    u64 cnt = 0;
    for (i64 base = s0; base < s1; base += EX_RANK_TILE) {
        const int len = (int)(s1 - base < EX_RANK_TILE ? s1 - base : EX_RANK_TILE);
        __syncthreads();
        for (int k = threadIdx.x; k < len; k += EX_RANK_THREADS) heads[k] = H[base + k];
        __syncthreads();
        for (int k0 = 0; k0 < len; k0 += EX_RANK_GROUP) {           // every lane of the wave, live or not: the walks are shared
            const int k1 = k0 + EX_RANK_GROUP < len ? k0 + EX_RANK_GROUP : len;
            // the common case in a tight pass: equal heads count unless the tails say otherwise
            u32 ge = 0;
            bool tie = false;
#pragma unroll 8
            for (int k = k0; k < k1; ++k) {
                const u64 h = heads[k];
                ge += h >= hq ? 1u : 0u;
                tie |= h == hq;
            }
            cnt += ge;
            if (P >= T || !__ballot(live && tie)) continue;         // (a target's own head ties: its group comes here once)
            // some prefix does not decide: the tails, to the last entry; a pair that turns out smaller is taken off again
            for (int k = k0; k < k1; ++k) {
                const i64 i = base + k;
                const bool undecided = live && heads[k] == hq && i != iq;
                if (T - P <= EX_LANE_WALK) {                        // a short tail: every lane walks its own pair
                    if (undecided) {
                        const u32 *vi = E + i * T, *vq = E + iq * T;
                        for (i64 t = P; t < T; ++t) {
                            const u32 a = vi[t], c = vq[t];
                            if (a != c) {
                                cnt -= a < c ? 1u : 0u;
                                break;
                            }
                        }
                    }
                    continue;
                }
                // A long tail: the wave takes its open pairs in turn and compares 64 entries of the two rows at a time
                // (a walk by the one lane would be up to T dependent loads).
                u64 open = __ballot(undecided);
                while (open) {
                    const int owner = __ffsll((unsigned long long)open) - 1;
                    open &= open - 1;
                    const u32 *vi = E + i * T, *vo = E + (i64)__shfl((int)iq, owner) * T;  // iq < n < 2^31
                    int smaller = 0;                                // equal to the end counts
                    for (i64 t0 = P; t0 < T; t0 += 64) {
                        const i64 t = t0 + lane;
                        u32 a = 0, c = 0;
                        if (t < T) {
                            a = vi[t];
                            c = vo[t];
                        }
                        const u64 differ = __ballot(a != c);
                        if (differ) {
                            smaller = __shfl((int)(a < c), __ffsll((unsigned long long)differ) - 1);
                            break;
                        }
                    }
                    if (lane == owner) cnt -= (u32)smaller;
                }
            }
        }
    }
    if (live && cnt) atomicAdd(out + q, (unsigned long long)cnt);
}

// ---------------------------------------------------------------------------------------------- host
static inline int ex_field_bits(i64 n) {
    int b = 0;
    for (u64 v = (u64)(n - 1); v; v >>= 1) ++b;
    return b < 16 ? 16 : b;
}

// stage 2 as the consumer of stage 1's batches
struct ExtremityTransform final : RankImageConsumer {
    i64 n, T;
    u32 *E;
    ExtremityTransform(i64 n_, i64 T_, u32 *E_) : n(n_), T(T_), E(E_) {}
    int image32(const u32 *img, i64 row0, i64 rows, hipStream_t s) override { return launch_ex_transform<u32>(img, row0, rows, n, T, E, s); }
    int image64(const u64 *img, i64 row0, i64 rows, hipStream_t s) override { return launch_ex_transform<u64>(img, row0, rows, n, T, E, s); }
};

// E and H in front of stage 1, which takes the bytes they leave or is sized by its rows
ExtremalPlan extremal_plan(i64 T, i64 n, int route, PlanSize size) {
    const size_t fixed = align_up((size_t)n * T * 4, 256) + align_up((size_t)n * 8, 256);
    if (!size.rows) size.bytes = size.bytes > fixed ? size.bytes - fixed : 0;
    const PairImagePlan stage1 = pair_image_plan(T, n, route, size);
    return {stage1, fixed + stage1.bytes};
}

int launch_extremal_counts(const double *Y, i64 T, i64 n, const i64 *targets, i64 m, int route, i64 *out, void *ws,
                           size_t ws_bytes, hipStream_t s) {
    const ExtremalPlan plan = extremal_plan(T, n, route, PlanSize::of_bytes(ws_bytes));
    Carver cv(ws, ws_bytes);
    u32 *E = (u32 *)cv.take((size_t)n * T * 4);
    u64 *H = (u64 *)cv.take((size_t)n * 8);
    if (!E || !H) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_extremal_min_workspace_bytes)");
    ExtremityTransform transform(n, T, E);
    int rc = launch_rank_pair_images(plan.stage1, Y, T, n, transform, cv.take(plan.stage1.bytes), s);
    if (rc) return rc;

    int Tp = 2;
    while (Tp < T) Tp <<= 1;
    const int b = ex_field_bits(n), P = (int)(T < 64 / b ? T : 64 / b);
    const int threads = Tp <= EX_WAVE_KEYS ? 256 : (Tp / 4 > 1024 ? 1024 : Tp / 4);        // four keys a thread
    const int tpc = Tp <= EX_WAVE_KEYS ? 64 : threads, cpb = threads / tpc;
    hipLaunchKernelGGL(ex_sort_kernel, dim3((unsigned)((n + cpb - 1) / cpb)), dim3(threads), (size_t)cpb * Tp * 4, s, E, T, n, Tp,
                       tpc, b, P, H);
    SD_HIP(hipGetLastError());

    SD_HIP(hipMemsetAsync(out, 0, (size_t)m * 8, s));
    // the sample in chunks of whole units of EX_RANK_SPLIT heads, about eight workgroups per CU: a walk is a chain of
    // dependent loads, and other waves are what hides it
    const i64 gx = (m + EX_RANK_THREADS - 1) / EX_RANK_THREADS, units = (n + EX_RANK_SPLIT - 1) / EX_RANK_SPLIT;
    i64 split = ((i64)8 * device_cus() + gx - 1) / gx;
    split = split < 1 ? 1 : split > units ? units : split;
    const i64 chunk = (units + split - 1) / split * EX_RANK_SPLIT, gy = (n + chunk - 1) / chunk;
    hipLaunchKernelGGL(ex_rank_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(EX_RANK_THREADS), 0, s, H, E, T, n, P, targets, m,
                       chunk, (unsigned long long *)out);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

}  // namespace sd
