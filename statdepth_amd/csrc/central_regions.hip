// central_regions.hip -- K16: central regions, fence, outside counts and whiskers of the functional boxplot
// (Sun & Genton 2011; regions from any depth, Narisetty & Nair 2016).
//
// Definition.  n curves at T timepoints, time-major Y[t][i], no NaN.  Curve i carries one byte level[i]; region l is
// { i : level[i] <= l }, l = 0 .. L - 1 (L <= 8), a level >= L is in no region.  Per timepoint t
//   env[l][0][t] = min, env[l][1][t] = max of Y[t][i] over region l           (+inf / -inf for an empty region),
//   r = upper - lower, w = F * r, lf = lower - w, uf = upper + w of region `box`    (four rounded operations),
//   outside[i][0] = #{ t : Y[t][i] < lf[t] },  outside[i][1] = #{ t : Y[t][i] > uf[t] }   (a NaN fence flags nobody),
//   whisker[0][t] / whisker[1][t] = min / max over the curves with outside == (0, 0).
//
// Two routes, every dependency between passes a kernel boundary, every loop bounded by T or n:
//   row-resident   n <= CR_ROW_CAPACITY: a workgroup holds R whole rows of Y in registers, VPT values of each row a thread
//                  (VPT * R = 16; thread x owns the curves x, x + threads, ...: their level bytes are read once).  Per row
//                  and exact level the thread's values, the wave (shuffles) and the workgroup (LDS) are reduced to one
//                  min / max; one thread per row accumulates the levels upward, writes env and the fence, the fence goes
//                  back through LDS and every thread compares the values it still holds.  The below / above counts stay
//                  in registers over the workgroup's rows and are added to `outside` once at the end (integer atomics:
//                  the same sums in any order).  Y is read once;
//   column blocks  any n: the same reduction over a block of CR_BLOCK_COLS curves writes the block's min / max per (row,
//                  level) to the workspace, cr_combine_kernel folds the blocks of a row into env and the fence, and
//                  cr_count_kernel reads Y again for the counts.
// The whiskers are the same envelope code once more with one level, "outside == (0, 0)", in a launch behind the counts.
#include "sd_common.h"

namespace sd {

constexpr int CR_MAX_THREADS = 1024;
constexpr int CR_VALUES = 16;                                      // values of Y a thread holds: VPT columns x R rows
constexpr int CR_SMALL_THREADS = 512;                              // workgroups of up to this size share a CU
constexpr int CR_BLOCK_VPT = 16;                                   // the column-block route: 512 threads x 16 curves ...
constexpr int CR_BLOCK_COLS = CR_SMALL_THREADS * CR_BLOCK_VPT;     // ... = 8192 curves a block, a row at a time: two a CU
constexpr int CR_COMBINE_ROWS = 4;                                 // rows (waves) of a combine workgroup
constexpr int CR_COUNT_THREADS = 256;
constexpr int CR_NONE = 15;                                        // the 4-bit level of a curve in no region

static_assert(CR_ROW_CAPACITY == (i64)CR_MAX_THREADS * CR_VALUES, "one row in the registers of one workgroup");

__device__ __forceinline__ double cr_wave_min(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ double cr_wave_max(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d));
    return v;
}

// the fence of one row from the box region's envelope: four rounded operations, never contracted
__device__ __forceinline__ void cr_fence(double lower, double upper, double factor, double &lf, double &uf) {
    const double r = __dsub_rn(upper, lower);
    const double w = __dmul_rn(factor, r);
    lf = __dsub_rn(lower, w);
    uf = __dadd_rn(upper, w);
}

// Shared memory: part[R][L][2][waves], red[R][L][2], fen[R][2] doubles.
//
// BLOCKS = false (row-resident; grid.x workgroups share the batches of R rows): env, and with box >= 0 the fence (to
// `fence` when not null) and the counts (added to `outside` when not null).
// BLOCKS = true (blockIdx.x = column block, grid.y workgroups share the batches): partial[(t * ncb + cb) * 2L + 2l + side].
// mask != null: the level of curve i is 0 where mask[i] == (0, 0) and none otherwise (the whisker pass; `level` unused).
template <int VPT, int R, bool BLOCKS>
__global__ __launch_bounds__(CR_MAX_THREADS) void cr_rows_kernel(const double *__restrict__ Y, i64 T, i64 n,
                                                                 const uint8_t *__restrict__ level,
                                                                 const int32_t *__restrict__ mask, int L, int box, double factor,
                                                                 double *__restrict__ env, double *__restrict__ fence,
                                                                 int32_t *__restrict__ outside, double *__restrict__ partial) {
    extern __shared__ double cr_lds[];
    const int threads = blockDim.x, waves = threads >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *part = cr_lds, *red = part + (size_t)R * L * 2 * waves, *fen = red + R * L * 2;
    const i64 cb = BLOCKS ? blockIdx.x : 0, ncb = BLOCKS ? gridDim.x : 1;
    const i64 g0 = BLOCKS ? blockIdx.y : blockIdx.x, gstep = BLOCKS ? gridDim.y : gridDim.x;
    const u32 col0 = (u32)(cb * ((i64)threads * VPT)) + threadIdx.x; // the thread's curves: col0 + k * threads (below 2^31 + 8192)
    const double INF = __longlong_as_double(0x7FF0000000000000ll), QNAN = __longlong_as_double(0x7FF8000000000000ll);

    u64 lv = 0;                                                     // 4 bits a curve
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const u32 i = col0 + (u32)(k * threads);
        int l = CR_NONE;
        if (i < n) {
            if (mask) l = (mask[2 * (i64)i] | mask[2 * (i64)i + 1]) ? CR_NONE : 0;
            else l = level[i] < L ? level[i] : CR_NONE;
        }
        lv |= (u64)l << (4 * k);
    }
    int below[VPT], above[VPT];
#pragma unroll
    for (int k = 0; k < VPT; ++k) below[k] = above[k] = 0;
    const bool counting = !BLOCKS && box >= 0 && outside != nullptr;

    const i64 batches = (T + R - 1) / R;
    for (i64 b = g0; b < batches; b += gstep) {
        const i64 t0 = b * R;
        double v[R][VPT];                                           // NaN where there is no row or no curve: compares false
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < VPT; ++k) {
                const u32 i = col0 + (u32)(k * threads);
                v[r][k] = (t0 + r < T && i < n) ? Y[(t0 + r) * n + i] : QNAN;
            }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            for (int l = 0; l < L; ++l) {
                double mn = INF, mx = -INF;                         // the identities, also for lanes past n
#pragma unroll
                for (int k = 0; k < VPT; ++k) {
                    const bool in = (int)((lv >> (4 * k)) & 15) == l;
                    mn = in ? fmin(mn, v[r][k]) : mn;
                    mx = in ? fmax(mx, v[r][k]) : mx;
                }
                mn = cr_wave_min(mn);
                mx = cr_wave_max(mx);
                if (lane == 0) {
                    part[((r * L + l) * 2 + 0) * waves + wave] = mn;
                    part[((r * L + l) * 2 + 1) * waves + wave] = mx;
                }
            }
        }
        __syncthreads();
        for (int item = threadIdx.x; item < R * L * 2; item += threads) {         // item = (r * L + l) * 2 + side
            const double *p = part + (size_t)item * waves;
            double a = p[0];
            if (item & 1) for (int w = 1; w < waves; ++w) a = fmax(a, p[w]);
            else for (int w = 1; w < waves; ++w) a = fmin(a, p[w]);
            const int r = item / (2 * L);
            if (BLOCKS) {
                if (t0 + r < T) partial[((t0 + r) * ncb + cb) * (2 * L) + (item - r * 2 * L)] = a;
            } else {
                red[item] = a;
            }
        }
        if (BLOCKS) {
            __syncthreads();                                        // part is written again by the next batch
            continue;
        }
        __syncthreads();
        if (threadIdx.x < R && t0 + threadIdx.x < T) {              // one thread a row: the levels upward
            const int r = threadIdx.x;
            const i64 t = t0 + r;
            double lo = INF, hi = -INF;
            for (int l = 0; l < L; ++l) {
                lo = fmin(lo, red[(r * L + l) * 2]);
                hi = fmax(hi, red[(r * L + l) * 2 + 1]);
                env[(i64)(2 * l) * T + t] = lo;
                env[(i64)(2 * l + 1) * T + t] = hi;
                if (l == box) {
                    double lf, uf;
                    cr_fence(lo, hi, factor, lf, uf);
                    fen[2 * r] = lf;
                    fen[2 * r + 1] = uf;
                    if (fence) {
                        fence[t] = lf;
                        fence[T + t] = uf;
                    }
                }
            }
        }
        if (counting) {
            __syncthreads();
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (t0 + r < T) {                                   // (fen of a missing row is not written)
                    const double lf = fen[2 * r], uf = fen[2 * r + 1];
#pragma unroll
                    for (int k = 0; k < VPT; ++k) {
                        below[k] += v[r][k] < lf ? 1 : 0;
                        above[k] += v[r][k] > uf ? 1 : 0;
                    }
                }
            }
        }
        // the next batch writes part behind two barriers of this one, red and fen behind its own first barrier
    }
    if (counting) {
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            const u32 i = col0 + (u32)(k * threads);
            if (i < n) {
                if (below[k]) atomicAdd(outside + 2 * (i64)i, below[k]);
                if (above[k]) atomicAdd(outside + 2 * (i64)i + 1, above[k]);
            }
        }
    }
}

// the column blocks of a row folded into env and, with box >= 0, the fence (fence: 2 x T, never null then); a wave a row
__global__ __launch_bounds__(64 * CR_COMBINE_ROWS) void cr_combine_kernel(const double *__restrict__ partial, i64 T, i64 ncb,
                                                                          int L, int box, double factor,
                                                                          double *__restrict__ env, double *__restrict__ fence) {
    const i64 t = (i64)blockIdx.x * CR_COMBINE_ROWS + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;                                             // the whole wave
    const double INF = __longlong_as_double(0x7FF0000000000000ll);
    const double *p = partial + t * ncb * (2 * L);
    double lo = INF, hi = -INF;
    for (int l = 0; l < L; ++l) {
        double mn = INF, mx = -INF;
        for (i64 c = lane; c < ncb; c += 64) {
            mn = fmin(mn, p[c * (2 * L) + 2 * l]);
            mx = fmax(mx, p[c * (2 * L) + 2 * l + 1]);
        }
        lo = fmin(lo, cr_wave_min(mn));
        hi = fmax(hi, cr_wave_max(mx));
        if (lane == 0) {
            env[(i64)(2 * l) * T + t] = lo;
            env[(i64)(2 * l + 1) * T + t] = hi;
            if (l == box) {
                double lf, uf;
                cr_fence(lo, hi, factor, lf, uf);
                fence[t] = lf;
                fence[T + t] = uf;
            }
        }
    }
}

// outside[i] += the below / above counts of curve i over the blockIdx.y-th chunk of rows
__global__ __launch_bounds__(CR_COUNT_THREADS) void cr_count_kernel(const double *__restrict__ Y, i64 T, i64 n,
                                                                    const double *__restrict__ fence, i64 chunk,
                                                                    int32_t *__restrict__ outside) {
    const i64 i = (i64)blockIdx.x * CR_COUNT_THREADS + threadIdx.x;
    if (i >= n) return;
    const i64 r0 = (i64)blockIdx.y * chunk, r1 = r0 + chunk < T ? r0 + chunk : T;
    int below = 0, above = 0;
#pragma unroll 4
    for (i64 t = r0; t < r1; ++t) {
        const double x = Y[t * n + i];
        below += x < fence[t] ? 1 : 0;
        above += x > fence[T + t] ? 1 : 0;
    }
    if (below) atomicAdd(outside + 2 * i, below);
    if (above) atomicAdd(outside + 2 * i + 1, above);
}

// ---------------------------------------------------------------------------------------------- host
static inline i64 cr_blocks(i64 n) { return (n + CR_BLOCK_COLS - 1) / CR_BLOCK_COLS; }

static size_t cr_partial_bytes(i64 T, i64 n, int L) {
    return n > CR_ROW_CAPACITY ? align_up((size_t)T * cr_blocks(n) * L * 16, 256) : 0;
}

size_t central_regions_workspace_bytes(i64 T, i64 n, int L) {
    return align_up((size_t)T * 16, 256) + align_up((size_t)n * 8, 256) + cr_partial_bytes(T, n, L);
}

template <int VPT, int R, bool BLOCKS>
static int cr_launch_rows(dim3 grid, int threads, const double *Y, i64 T, i64 n, const uint8_t *level, const int32_t *mask, int L,
                          int box, double factor, double *env, double *fence, int32_t *outside, double *partial, hipStream_t s) {
    const size_t lds = ((size_t)R * L * 2 * (threads / 64) + (size_t)R * L * 2 + (size_t)R * 2) * 8;
    hipLaunchKernelGGL((cr_rows_kernel<VPT, R, BLOCKS>), grid, dim3(threads), lds, s, Y, T, n, level, mask, L, box, factor, env,
                       fence, outside, partial);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

// env (L x 2 x T) of the levels (or of mask: one level), and with box >= 0 the fence into `fence` (never null then) and,
// where `outside` is not null, the counts added to it
static int cr_pass(const double *Y, i64 T, i64 n, const uint8_t *level, const int32_t *mask, int L, int box, double factor,
                   double *env, double *fence, int32_t *outside, double *partial, hipStream_t s) {
    const int cus = device_cus();
    if (n <= CR_ROW_CAPACITY) {
        // up to 8192 curves the workgroup stays at 512 threads, so that two or three share a CU and one loads while another
        // reduces; above, a row takes 16 values a thread and up to 1024 threads, one workgroup a CU
        int vpt = 1;
        while (vpt < CR_VALUES && (i64)vpt * CR_SMALL_THREADS < n) vpt <<= 1;
        const int threads = (int)(((n + vpt - 1) / vpt + 63) / 64 * 64), R = CR_VALUES / vpt;
        // as many workgroups as are resident at once (waves a CU holds at the variant's register count), each looping over
        // its batches: a workgroup a batch reads the levels and adds its counts once per batch and measured slower
        const int cu_waves = vpt == 1 ? 28 : vpt == 2 ? 24 : vpt == 4 ? 20 : 16, wg_waves = threads / 64;
        const i64 batches = (T + R - 1) / R, want = (i64)(cu_waves / wg_waves > 0 ? cu_waves / wg_waves : 1) * cus;
        const dim3 grid((unsigned)(batches < want ? batches : want));
        switch (vpt) {
            case 1: return cr_launch_rows<1, 16, false>(grid, threads, Y, T, n, level, mask, L, box, factor, env, fence, outside, nullptr, s);
            case 2: return cr_launch_rows<2, 8, false>(grid, threads, Y, T, n, level, mask, L, box, factor, env, fence, outside, nullptr, s);
            case 4: return cr_launch_rows<4, 4, false>(grid, threads, Y, T, n, level, mask, L, box, factor, env, fence, outside, nullptr, s);
            case 8: return cr_launch_rows<8, 2, false>(grid, threads, Y, T, n, level, mask, L, box, factor, env, fence, outside, nullptr, s);
            default: return cr_launch_rows<16, 1, false>(grid, threads, Y, T, n, level, mask, L, box, factor, env, fence, outside, nullptr, s);
        }
    }
    constexpr int R = CR_VALUES / CR_BLOCK_VPT;
    const i64 ncb = cr_blocks(n), batches = (T + R - 1) / R;
    i64 gy = ((i64)8 * cus + ncb - 1) / ncb;                         // about eight workgroups a CU ...
    gy = gy > batches ? batches : gy;
    gy = gy > 65535 ? 65535 : gy;
    const i64 each = (batches + gy - 1) / gy;                       // ... with the same number of batches each
    gy = (batches + each - 1) / each;
    int rc = cr_launch_rows<CR_BLOCK_VPT, R, true>(dim3((unsigned)ncb, (unsigned)gy), CR_SMALL_THREADS, Y, T, n, level, mask, L,
                                                   box, factor, nullptr, nullptr, nullptr, partial, s);
    if (rc) return rc;
    hipLaunchKernelGGL(cr_combine_kernel, dim3((unsigned)((T + CR_COMBINE_ROWS - 1) / CR_COMBINE_ROWS)), dim3(64 * CR_COMBINE_ROWS),
                       0, s, partial, T, ncb, L, box, factor, env, fence);
    SD_HIP(hipGetLastError());
    if (box >= 0 && outside) {
        const i64 gx = (n + CR_COUNT_THREADS - 1) / CR_COUNT_THREADS;
        i64 chunks = ((i64)8 * cus + gx - 1) / gx;
        chunks = chunks > T ? T : chunks;
        chunks = chunks > 65535 ? 65535 : chunks;
        const i64 chunk = (T + chunks - 1) / chunks;
        hipLaunchKernelGGL(cr_count_kernel, dim3((unsigned)gx, (unsigned)((T + chunk - 1) / chunk)), dim3(CR_COUNT_THREADS), 0, s, Y,
                           T, n, fence, chunk, outside);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

int launch_central_regions(const double *Y, i64 T, i64 n, const uint8_t *level, int L, int box, double factor, double *env,
                           double *fence, int32_t *outside, double *whisker, void *ws, size_t ws_bytes, hipStream_t s) {
    Carver cv(ws, ws_bytes);
    double *ws_fence = (double *)cv.take((size_t)T * 16);
    int32_t *ws_outside = (int32_t *)cv.take((size_t)n * 8);
    double *partial = n > CR_ROW_CAPACITY ? (double *)cv.take((size_t)T * cr_blocks(n) * L * 16) : nullptr;
    if (!cv.ok()) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_central_regions_workspace_bytes)");
    const bool fenced = box >= 0 && (fence || outside || whisker);
    int32_t *counts = outside ? outside : (whisker ? ws_outside : nullptr);
    if (counts) SD_HIP(hipMemsetAsync(counts, 0, (size_t)n * 8, s));
    int rc = cr_pass(Y, T, n, level, nullptr, L, fenced ? box : -1, factor, env, fenced ? (fence ? fence : ws_fence) : nullptr,
                     counts, partial, s);
    if (rc || !whisker) return rc;
    return cr_pass(Y, T, n, nullptr, counts, 1, -1, 0.0, whisker, nullptr, nullptr, partial, s);
}

}  // namespace sd
