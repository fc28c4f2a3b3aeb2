// curve_dist.hip -- K20: squared L2 distances between curves, the k-th smallest of them, and the h-modal sums of Cuevas,
// Febrero & Fraiman (2006).
//
// Definition.  n curves at T timepoints, time-major Y[t][i], finite, |y| <= 2^480.  For a target x (a sample curve i, or an
// external curve, a column of Q) and a sample curve j, one accumulator over ascending t from +0.0:
//   d = x[t] - Y[t][j];   acc = fma(d, d, acc)                       two rounded operations per timepoint
// D2 = acc.  Nothing is split over t, there is no Gram form and no MFMA: (-d) * (-d) = d * d exactly, so D2[i][j] and D2[j][i]
// hold the same bits; the diagonal is +0.0; a subnormal product is kept by the fma.
// h-modal sum of a target: S = sum_j exp(-(D2[j] * g)) over all n sample curves, g a double of the caller.  The order:
//   columns in tiles of 64, b = 0 .. ceil(n / 64) - 1; inside tile b, lane x = 0 .. 15 owns the columns
//     j(c, e) = 64 b + 32 c + 2 x + e,  c = 0 .. 1, e = 0 .. 1,
//   and adds its terms from +0.0 in ascending (c, e), a column j >= n adding nothing; the 16 lanes meet in a butterfly,
//     v = v + v[x ^ 1]; v = v + v[x ^ 2]; v = v + v[x ^ 4]; v = v + v[x ^ 8]
//   (both partners form the same sum, addition being commutative), which gives the tile's partial sum P[b];
//   S = ((P[0] + P[1]) + P[2]) + ...  from +0.0 in ascending b (cd_fold_kernel, one thread per target).
// The order depends on n alone: S of a target has the same bits whatever the target list, the layout of X or the workspace.
// k-th smallest of D2 over the pairs i < j (k 1-based): nonnegative doubles order like their 64-bit images, and the image is
// found from the top by a radix descent, digits of 11, 11, 11, 11, 11 and 9 bits: a pass counts, over the pairs whose image
// agrees with the prefix found so far, the values of the next digit (u32 atomics in LDS, then u64 atomics in global memory:
// integers, so the counts do not depend on any order), and cd_pick_kernel takes the digit that holds rank k, on the device.
//
// cd_tile_kernel<EPI>: one workgroup of 256 threads per (128 targets x 64 sample curves).  Both operand panels are staged in
// LDS in chunks of 16 timepoints (16 + 8 KiB); time-major rows keep the curve index contiguous, so neither needs a transpose
// (the targets' panel is gathered through the target list, or read from Q).  Thread (x, y) = (tid & 15, tid >> 4) holds an
// 8 x 4 register tile: the rows 8 y + r and the columns 32 c + 2 x + e, so a wave reads 16 consecutive 16-byte words of the
// sample panel (broadcast over its four y) and four runs of the targets' panel.  Several workgroups share a CU, and one
// fetches its chunk while the others compute; there is no register prefetch of the next chunk.
// Why 8 x 4 (tools/experiments/curve_dist_tiles.hip): by the per-clock figures -- a wave64 fp64
// operation holds a SIMD for 4 cycles, the LDS gives 128 B a clock to the CU -- a 4 x 4 tile (64 B read per 32 operations)
// would fill the LDS once all four SIMDs issue and an 8 x 8 tile would halve that.  Measured at 10 000 x 1 000, the tile
// is not what bounds the loop: 8 x 8 (178 VGPRs, 2 waves a SIMD) 8.47 ms, 4 x 4 (64 VGPRs, 8 waves) 8.04 ms, 8 x 4 and 4 x 8
// (108 VGPRs, 4 waves) 7.90 and 7.93 ms.  8 x 8 with a register prefetch on top spilled.
// The epilogue is a compile-time choice:
//   CD_STORE   D2 to out[q][j] (the m x n output, or the n x n slab of the selection, there the tiles with a pair i < j only);
//   CD_HMODAL  the tile's partial sums P[b] of its 128 targets to part[q - row0][b]; cd_fold_kernel adds them (no
//              floating-point atomics anywhere);
//   CD_HIST    the digits of the tile's pairs i < j into the histogram (the targets are the sample curves in order);
//   CD_WEIGHT  K21's weights w = 1 / sqrt(D2) (0.0 where D2 == 0.0; one correctly rounded root, one correctly rounded
//              division) to out[j][q - row0], sample-curve-major: the panel [j][q] that sp_sum_kernel (spatial_depth.hip)
//              stages.  All 128 target columns of a tile are written, those past the last target too (finite values that
//              nothing reads), so a batch's slab holds no byte that was not written.
// The selection keeps the n x n slab when the workspace holds it (cd_slab_hist_kernel re-reads it per pass) and otherwise
// recomputes the tiles in every pass; both count the same multiset of images, so the result is the same.
// The batch plan (curve_dist_plan): the h-modal partial sums are the only per-target workspace, 8 ceil(n / 64) bytes a target,
// in the blocks of curve_routes.h; the distances go straight to the output and the selection's workspace does not depend on
// the targets.
#include "curve_routes.h"

namespace sd {

constexpr int CD_TILE = CV_BLOCK, CD_COLS = 64;                     // targets (the plan's block) and sample curves of a tile
constexpr int CD_TK = 16, CD_THREADS = 256, CD_R = CD_TILE / 16, CD_C = CD_COLS / 16;
constexpr int CD_STORE = 0, CD_HMODAL = 1, CD_HIST = 2, CD_WEIGHT = 3;
constexpr int CD_BINS = 2048, CD_PASSES = 6;
constexpr int CD_STATE_WORDS = 32;                                  // prefix, k; the rest pads the region
constexpr size_t CD_PART_MAX = (size_t)256 << 20;                   // partial sums of a batch (recommended size and launch)
constexpr size_t CD_SLAB_MAX = (size_t)1 << 30;                     // the selection's slab: above it every pass recomputes

static inline i64 cd_tiles(i64 n) { return (n + CD_COLS - 1) / CD_COLS; }   // column tiles

// the digit of pass p lies at bits [shift, shift + bits)
static inline int cd_pass_shift(int p) { return p < 5 ? 53 - 11 * p : 0; }
static inline int cd_pass_bits(int p) { return p < 5 ? 11 : 9; }

__device__ __forceinline__ bool cd_counts(u64 v, u64 prefix, int top) { return top >= 64 || (v >> top) == (prefix >> top); }

// one timepoint of the register tile: As and Bs point at row k of the panels
__device__ __forceinline__ void cd_step(const double *__restrict__ As, const double *__restrict__ Bs, int x, int y,
                                        double (&acc)[CD_R][CD_C]) {
    double a[CD_R], b[CD_C];
#pragma unroll
    for (int r = 0; r < CD_R; r += 2) {
        const double2 v = *reinterpret_cast<const double2 *>(As + CD_R * y + r);
        a[r] = v.x, a[r + 1] = v.y;
    }
#pragma unroll
    for (int c = 0; c < CD_C / 2; ++c) {
        const double2 v = *reinterpret_cast<const double2 *>(Bs + 32 * c + 2 * x);
        b[2 * c] = v.x, b[2 * c + 1] = v.y;
    }
#pragma unroll
    for (int r = 0; r < CD_R; ++r)
#pragma unroll
        for (int c = 0; c < CD_C; ++c) {
            const double d = a[r] - b[c];
            acc[r][c] = fma(d, d, acc[r][c]);
        }
}

// Targets [q_first + 128 (blockIdx.x / nb) ...) x sample curves [64 (blockIdx.x % nb) ...).  P, ldp, targets: the targets'
// panel, value (t, q) = P[t * ldp + (targets ? targets[q] : q)].  q_end: one past the last target.  upper: only tiles that
// hold a pair q < j (CD_STORE for the slab; CD_HIST always).  out, row0, ldo: CD_STORE out[(q - row0) * ldo + j], CD_HMODAL
// out[(q - row0) * ldo + tile], CD_WEIGHT out[j * ldo + (q - row0)] (ldo a multiple of 128, row0 = q_first of the batch's
// first launch, out 16-byte aligned).  hist, state, shift, bits: CD_HIST.
template <int EPI>
__global__ __launch_bounds__(CD_THREADS, 2) void cd_tile_kernel(const double *__restrict__ Y, i64 T, i64 n, const double *__restrict__ P,
                                                             i64 ldp, const i64 *__restrict__ targets, i64 q_first, i64 q_end, i64 nb,
                                                             int upper, double g, double *__restrict__ out, i64 row0, i64 ldo,
                                                             u64 *__restrict__ hist, const u64 *__restrict__ state, int shift,
                                                             int bits) {
    __shared__ __attribute__((aligned(16))) double As[CD_TK][CD_TILE];
    __shared__ __attribute__((aligned(16))) double Bs[CD_TK][CD_COLS];
    const int tid = threadIdx.x, x = tid & 15, y = tid >> 4;
    const i64 cb = (i64)blockIdx.x % nb, q0 = q_first + (i64)blockIdx.x / nb * CD_TILE, j0 = cb * CD_COLS;
    if ((EPI == CD_HIST || upper) && q0 >= j0 + CD_COLS - 1) return;   // no pair q < j in the tile

    // a thread fetches one column of each panel: of the targets' at the rows (tid >> 7) + 2 l of a chunk, of the sample's at
    // the rows (tid >> 6) + 4 l
    const int col = tid & (CD_TILE - 1), k0 = tid >> 7, colb = tid & (CD_COLS - 1), kb0 = tid >> 6;
    const i64 qa = q0 + col, jb = j0 + colb;
    const double *pa = qa < q_end ? P + (targets ? targets[qa] : qa) : nullptr;
    const double *pb = jb < n ? Y + jb : nullptr;

    double acc[CD_R][CD_C];
#pragma unroll
    for (int r = 0; r < CD_R; ++r)
#pragma unroll
        for (int c = 0; c < CD_C; ++c) acc[r][c] = 0.0;

    for (i64 t0 = 0; t0 < T; t0 += CD_TK) {
        __syncthreads();                                            // the chunk before is consumed
#pragma unroll
        for (int l = 0; l < CD_TK / 2; ++l) {
            const int k = k0 + 2 * l;
            const i64 t = t0 + k;
            As[k][col] = pa && t < T ? pa[t * ldp] : 0.0;
        }
#pragma unroll
        for (int l = 0; l < CD_TK / 4; ++l) {
            const int k = kb0 + 4 * l;
            const i64 t = t0 + k;
            Bs[k][colb] = pb && t < T ? pb[t * n] : 0.0;
        }
        __syncthreads();
        const int rows = T - t0 < CD_TK ? (int)(T - t0) : CD_TK;
#pragma unroll 2
        for (int k = 0; k < rows; ++k) cd_step(As[k], Bs[k], x, y, acc);
    }

    if constexpr (EPI == CD_STORE) {
#pragma unroll
        for (int r = 0; r < CD_R; ++r) {
            const i64 q = q0 + CD_R * y + r;
            if (q >= q_end) continue;
            double *row = out + (q - row0) * ldo;
#pragma unroll
            for (int c = 0; c < CD_C; ++c) {
                const i64 j = j0 + 32 * (c >> 1) + 2 * x + (c & 1);
                if (j < n) row[j] = acc[r][c];
            }
        }
    } else if constexpr (EPI == CD_HMODAL) {
#pragma unroll
        for (int r = 0; r < CD_R; ++r) {
            double v = 0.0;
#pragma unroll
            for (int c = 0; c < CD_C; ++c) {
                const i64 j = j0 + 32 * (c >> 1) + 2 * x + (c & 1);
                if (j < n) v += exp(-(acc[r][c] * g));
            }
            v += __shfl_xor(v, 1);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 4);
            v += __shfl_xor(v, 8);
            const i64 q = q0 + CD_R * y + r;
            if (x == 0 && q < q_end) out[(q - row0) * ldo + cb] = v;
        }
    } else if constexpr (EPI == CD_WEIGHT) {
#pragma unroll
        for (int c = 0; c < CD_C; ++c) {
            const i64 j = j0 + 32 * (c >> 1) + 2 * x + (c & 1);
            if (j >= n) continue;
            double *col = out + j * ldo + (q0 - row0) + CD_R * y;
#pragma unroll
            for (int r = 0; r < CD_R; r += 2) {
                double2 w;
                w.x = acc[r][c] == 0.0 ? 0.0 : __ddiv_rn(1.0, __dsqrt_rn(acc[r][c]));
                w.y = acc[r + 1][c] == 0.0 ? 0.0 : __ddiv_rn(1.0, __dsqrt_rn(acc[r + 1][c]));
                *reinterpret_cast<double2 *>(col + r) = w;
            }
        }
    } else {
        __shared__ u32 lh[CD_BINS];
        for (int i = tid; i < CD_BINS; i += CD_THREADS) lh[i] = 0;
        __syncthreads();
        const u64 prefix = state[0];
        const int top = shift + bits;
        const u32 mask = (1u << bits) - 1;
#pragma unroll
        for (int r = 0; r < CD_R; ++r) {
            const i64 q = q0 + CD_R * y + r;
#pragma unroll
            for (int c = 0; c < CD_C; ++c) {
                const i64 j = j0 + 32 * (c >> 1) + 2 * x + (c & 1);
                const u64 v = (u64)__double_as_longlong(acc[r][c]);
                if (q < q_end && q < j && j < n && cd_counts(v, prefix, top)) atomicAdd(&lh[(u32)(v >> shift) & mask], 1u);
            }
        }
        __syncthreads();
        for (int i = tid; i < CD_BINS; i += CD_THREADS)
            if (lh[i]) atomicAdd(&hist[i], (u64)lh[i]);
    }
}

// out[q] = the partial sums of target q in ascending tile order
__global__ __launch_bounds__(256) void cd_fold_kernel(const double *__restrict__ part, i64 count, i64 nb, double *__restrict__ out) {
    const i64 q = (i64)blockIdx.x * 256 + threadIdx.x;
    if (q >= count) return;
    const double *p = part + q * nb;
    double s = 0.0;
    for (i64 b = 0; b < nb; ++b) s += p[b];
    out[q] = s;
}

// the histogram of a pass from the stored slab: a workgroup takes the rows blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(256) void cd_slab_hist_kernel(const double *__restrict__ slab, i64 n, u64 *__restrict__ hist,
                                                           const u64 *__restrict__ state, int shift, int bits) {
    __shared__ u32 lh[CD_BINS];
    const int tid = threadIdx.x;
    const u64 prefix = state[0];
    const int top = shift + bits;
    const u32 mask = (1u << bits) - 1;
    for (i64 i = blockIdx.x; i + 1 < n; i += gridDim.x) {
        for (int b = tid; b < CD_BINS; b += 256) lh[b] = 0;
        __syncthreads();
        const double *row = slab + i * n;
        for (i64 j = i + 1 + tid; j < n; j += 256) {
            const u64 v = (u64)__double_as_longlong(row[j]);
            if (cd_counts(v, prefix, top)) atomicAdd(&lh[(u32)(v >> shift) & mask], 1u);
        }
        __syncthreads();
        for (int b = tid; b < CD_BINS; b += 256)
            if (lh[b]) atomicAdd(&hist[b], (u64)lh[b]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void cd_select_init_kernel(u64 *__restrict__ hist, u64 *__restrict__ state, u64 k) {
    for (int b = threadIdx.x; b < CD_BINS; b += 256) hist[b] = 0;
    if (threadIdx.x < CD_STATE_WORDS) state[threadIdx.x] = threadIdx.x == 1 ? k : 0;
}

// The digit that holds rank k among the pairs counted: state = (prefix | digit << shift, k - the pairs in lower digits); the
// histogram is zeroed for the next pass; after the last pass the prefix is the image of the result.
__global__ __launch_bounds__(256) void cd_pick_kernel(u64 *__restrict__ hist, u64 *__restrict__ state, int shift, int last,
                                                      double *__restrict__ out) {
    constexpr int PER = CD_BINS / 256;
    __shared__ u64 part[256];
    __shared__ u64 before;
    __shared__ int owner;
    const int tid = threadIdx.x;
    u64 c[PER], s = 0;
#pragma unroll
    for (int b = 0; b < PER; ++b) s += c[b] = hist[tid * PER + b];
    part[tid] = s;
    __syncthreads();
    const u64 k = state[1];
    if (tid == 0) {
        u64 cum = 0;
        int w = 0;
        for (; w < 255 && cum + part[w] < k; ++w) cum += part[w];
        owner = w, before = cum;
    }
    __syncthreads();
    if (tid == owner) {
        u64 cum = before;
        int b = 0;
        for (; b < PER - 1 && cum + c[b] < k; ++b) cum += c[b];
        const u64 prefix = state[0] | (u64)(tid * PER + b) << shift;
        state[0] = prefix;
        state[1] = k - cum;
        if (last) *out = __longlong_as_double((long long)prefix);
    }
#pragma unroll
    for (int b = 0; b < PER; ++b) hist[tid * PER + b] = 0;
}

// ---------------------------------------------------------------------------------------------- the batch plan
static inline size_t cd_block_bytes(i64 n) { return (size_t)CD_TILE * (size_t)cd_tiles(n) * 8; }   // partial sums of 128 targets
static inline size_t cd_select_fixed() { return align_up((size_t)(CD_BINS + CD_STATE_WORDS) * 8, 256); }

CurveDistPlan curve_dist_plan(int what, i64 n, i64 m, PlanSize size) {
    CurveDistPlan p{what, 0, false, 0};
    if (what == CD_WHAT_SQDIST) {
        p.targets = m;
    } else if (what == CD_WHAT_HMODAL) {
        const size_t pb = cd_block_bytes(n);
        const TargetBlocks b = target_block_plan(m, size, pb, pb, CD_PART_MAX);
        if (b.blocks < 1) return p;
        p.targets = b.targets;
        p.bytes = align_up((size_t)b.blocks * pb, 256);
    } else {
        const size_t fixed = cd_select_fixed(), slab = (size_t)n * (size_t)n * 8;
        const bool fits = slab <= CD_SLAB_MAX;
        if (size.rows) p.slab = fits && size.rows >= n;
        else if (size.bytes < fixed) return p;
        else p.slab = fits && size.bytes >= fixed + slab;
        p.targets = n;
        p.bytes = fixed + (p.slab ? align_up(slab, 256) : 0);
    }
    return p;
}

// ---------------------------------------------------------------------------------------------- host
// the tiles of the targets [q_begin, q_end) of the m that sel names, nb tiles a target block
template <int EPI>
static int cd_launch_tiles(const double *Y, i64 T, i64 n, CurveSel sel, i64 m, i64 q_begin, i64 q_end, int upper, double g, double *out,
                           i64 row0, i64 ldo, u64 *hist, const u64 *state, int pass, hipStream_t s) {
    const i64 nb = cd_tiles(n);
    return for_block_launches(q_begin, q_end, nb, [&](i64 q, i64 tb) -> int {
        hipLaunchKernelGGL(cd_tile_kernel<EPI>, dim3((unsigned)(tb * nb)), dim3(CD_THREADS), 0, s, Y, T, n, sel.panel(Y), sel.ld(n, m),
                           sel.targets, q, q_end, nb, upper, g, out, row0, ldo, hist, state, cd_pass_shift(pass), cd_pass_bits(pass));
        SD_HIP(hipGetLastError());
        return SD_OK;
    });
}

int launch_curve_sqdist(const double *Y, i64 T, i64 n, CurveSel sel, i64 m, double *out, hipStream_t s) {
    return cd_launch_tiles<CD_STORE>(Y, T, n, sel, m, 0, m, 0, 0.0, out, 0, n, nullptr, nullptr, 0, s);
}

int launch_hmodal_sums(const double *Y, i64 T, i64 n, CurveSel sel, i64 m, double g, double *out, void *ws, size_t ws_bytes,
                       hipStream_t s) {
    const CurveDistPlan plan = curve_dist_plan(CD_WHAT_HMODAL, n, m, PlanSize::of_bytes(ws_bytes));
    Carver cv(ws, ws_bytes);
    double *part = plan.targets > 0 ? (double *)cv.take(plan.bytes) : nullptr;
    if (!part) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_curve_sqdist_min_workspace_bytes)");
    const i64 nb = cd_tiles(n);
    return for_target_batches(m, plan.targets, [&](i64 q, i64 count) -> int {
        int rc = cd_launch_tiles<CD_HMODAL>(Y, T, n, sel, m, q, q + count, 0, g, part, q, nb, nullptr, nullptr, 0, s);
        if (rc) return rc;
        hipLaunchKernelGGL(cd_fold_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, part, count, nb, out + q);
        SD_HIP(hipGetLastError());
        return SD_OK;
    });
}

// K21's pass 1: the weights of the targets [q_begin, q_end) into W[j * ldw + (q - q_begin)]
int launch_curve_weights(const double *Y, i64 T, i64 n, CurveSel sel, i64 m, i64 q_begin, i64 q_end, double *W, i64 ldw, hipStream_t s) {
    return cd_launch_tiles<CD_WEIGHT>(Y, T, n, sel, m, q_begin, q_end, 0, 0.0, W, q_begin, ldw, nullptr, nullptr, 0, s);
}

// K22's external rows: the distances of the targets [q_begin, q_end) of the m columns of Q into out[(q - q_begin) * n + j]
int launch_curve_sqdist_rows(const double *Y, i64 T, i64 n, const double *Q, i64 m, i64 q_begin, i64 q_end, double *out, hipStream_t s) {
    return cd_launch_tiles<CD_STORE>(Y, T, n, select_columns(Q), m, q_begin, q_end, 0, 0.0, out, q_begin, n, nullptr, nullptr, 0, s);
}

int launch_curve_sqdist_select(const double *Y, i64 T, i64 n, u64 k, double *out, void *ws, size_t ws_bytes, hipStream_t s) {
    const CurveDistPlan plan = curve_dist_plan(CD_WHAT_SELECT, n, n, PlanSize::of_bytes(ws_bytes));
    Carver cv(ws, ws_bytes);
    u64 *hist = plan.targets > 0 ? (u64 *)cv.take(cd_select_fixed()) : nullptr;
    double *slab = hist && plan.slab ? (double *)cv.take((size_t)n * (size_t)n * 8) : nullptr;
    if (!hist || (plan.slab && !slab)) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_curve_sqdist_min_workspace_bytes)");
    u64 *state = hist + CD_BINS;
    const CurveSel all = select_sample(nullptr);
    hipLaunchKernelGGL(cd_select_init_kernel, dim3(1), dim3(256), 0, s, hist, state, k);
    SD_HIP(hipGetLastError());
    if (slab) {
        int rc = cd_launch_tiles<CD_STORE>(Y, T, n, all, n, 0, n, 1, 0.0, slab, 0, n, nullptr, nullptr, 0, s);
        if (rc) return rc;
    }
    for (int pass = 0; pass < CD_PASSES; ++pass) {
        if (slab) {
            const unsigned grid = (unsigned)(n - 1 < 2048 ? n - 1 : 2048);
            hipLaunchKernelGGL(cd_slab_hist_kernel, dim3(grid), dim3(256), 0, s, slab, n, hist, state, cd_pass_shift(pass),
                               cd_pass_bits(pass));
            SD_HIP(hipGetLastError());
        } else {
            int rc = cd_launch_tiles<CD_HIST>(Y, T, n, all, n, 0, n, 1, 0.0, nullptr, 0, 0, hist, state, pass, s);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(cd_pick_kernel, dim3(1), dim3(256), 0, s, hist, state, cd_pass_shift(pass), pass == CD_PASSES - 1 ? 1 : 0, out);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

}  // namespace sd
