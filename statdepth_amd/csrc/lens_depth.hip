// lens_depth.hip -- K22: the lune depths of curves and point clouds on K20's matrix of squared L2 distances: the lens depth
// (Liu & Modarres 2011; Kleindessner & von Luxburg 2017; Geenens, Nieto-Reyes & Francisci 2023), the spherical depth (Elmore,
// Hettmansperger & Xuan 2006) and the beta-skeleton depth that joins them (Yang & Modarres 2018).
//
// Definition.  D2 is K20's number on K20's bits (curve_dist.hip): symmetric, +0.0 diagonal, subnormal squares kept.  For a
// target x (a sample curve, or an external curve, a column of Q) and the sample curves i < j:
//   a = D2(x, x_i);  b = D2(x, x_j);  c = D2(x_i, x_j);
//   t1 = kappa * b;  s1 = a + t1;  t2 = kappa * a;  s2 = b + t2       four separately rounded operations (__dmul_rn, __dadd_rn)
//   in = (s1 <= c) && (s2 <= c)
// G(x) = #{i < j : in}, an integer; out = G.  kappa = 2 / beta - 1 in [-1, 1] is the caller's double; the depth is G / C(n, 2).
// Three compile-time forms give the same integers where they overlap:
//   LN_LENS     kappa == 0.0:  a <= c && b <= c;
//   LN_SPHERE   kappa == 1.0:  __dadd_rn(a, b) <= c, one test, the addition commuting bitwise;
//   LN_GENERAL  any kappa, as written above (algo = 1 forces it: the cross-check of the other two).
// No index is special-cased: a sample target's own pairs (a = 0, c = b) satisfy the predicate and count, coincident curves
// (c = 0) count only for a coincident target (at kappa = -1 for every target: a - a <= 0).  D2 < 2^993, so s < 2^994 and
// nothing overflows.  The counts are integers added with integer atomics: they do not depend on any order, on the tiles, the
// target list, the layout of X or the workspace.
//
// Stage 1: the whole n x n matrix D through K20's tile kernel and its store epilogue (launch_curve_sqdist), and for external
// targets the rows A = D2(q, .) of a batch (launch_curve_sqdist_rows).  A sample target's row is D[targets[q]]: nothing is
// computed twice.
// Stage 2, lens_count_kernel<FORM>: one workgroup of 256 threads per (128 targets x the 64 sample curves i of tile I x a span
// of tiles J >= I of 64 sample curves j).  Thread (x, y) = (tid & 15, tid >> 4) holds the targets 8 y + r and the curves
// i(c) = 64 I + 32 (c >> 1) + 2 x + (c & 1): a register tile of 8 x 4 values of a, constant over the j loop (LN_GENERAL: and
// as many of kappa * a).  j is streamed in chunks of 16 through LDS: c as the rows D[j][i] of the symmetric matrix (so no
// transpose; 8 KiB) and the targets' b = A[q][j], transposed while staging (16 rows of 128 + 2 doubles: 16-byte reads stay
// aligned and the 16 lanes that write one target's 16 values hit 16 different bank pairs).  Per j a thread reads 8 b and 4 c
// for 32 triples.  Only the chunks of tile J == I need the mask i < j, and they run a loop of their own.  A curve i >= n or a
// target past the last has a = +inf, which fails the predicate in every form; j stops at n.  Per triple the lens form is two
// compares, a scalar and, and an add with carry-in; the spherical form an addition, a compare and the add with carry-in
// (profiles/r11_valu_rate.txt: a 64-bit compare issues at the rate of a 32-bit one, a select would cost more than the carry):
// 3 vector instructions a triple in both, 5.25 in the general form.  A scheduling barrier behind every eight triples keeps
// the compares next to their adds; without it the scheduler hoisted the compares of a whole j and spilled their masks to VGPR
// lanes inside the loop.
// Per-lane counters are 32-bit: a lane adds at most 4 n < 2^32.  The 16 lanes of a target meet in a butterfly and one lane
// adds the sum into out[q] (u64 atomic).  The span of J tiles of a workgroup is the launcher's choice (lens_span): whole rows
// of tiles where that still gives the device thousands of workgroups, shorter spans otherwise; workgroups whose span lies
// below the diagonal leave at once.  No workgroup waits for another.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; profiles/lens_depth_resources.txt), no scratch and no
// spill in any of them, 25 856 B of LDS:
//   lens_count_kernel<LN_LENS>     129 VGPRs, 3 waves a SIMD
//   lens_count_kernel<LN_SPHERE>   131 VGPRs, 3 waves a SIMD
//   lens_count_kernel<LN_GENERAL>  211 VGPRs, 2 waves a SIMD   (the second register tile, kappa * a)
// The plan (lens_plan): the matrix, 8 n^2 bytes, then the rows of a batch of external targets in the blocks of curve_routes.h;
// sample targets use no rows.
#include "curve_routes.h"

namespace sd {

constexpr int LN_TILE = CV_BLOCK, LN_COLS = 64;                     // targets of a block; sample curves of a tile (i and j alike)
constexpr int LN_JK = 16, LN_THREADS = 256, LN_R = LN_TILE / 16, LN_C = LN_COLS / 16;
constexpr int LN_LDB = LN_TILE + 2;                                 // row of the targets' panel in LDS
constexpr int LN_LENS = 0, LN_SPHERE = 1, LN_GENERAL = 2;
constexpr size_t LN_ROWS_MAX = (size_t)1 << 30;                     // external rows of a batch (recommended size and launch)
constexpr i64 LN_GROUPS_WANTED = 8192;                              // lens_span: workgroups (half of them empty) to aim for

static inline i64 ln_tiles(i64 n) { return (n + LN_COLS - 1) / LN_COLS; }

template <int FORM>
__device__ __forceinline__ bool ln_in(double a, double ka, double b, double kb, double c) {
    if constexpr (FORM == LN_LENS) return a <= c && b <= c;
    else if constexpr (FORM == LN_SPHERE) return __dadd_rn(a, b) <= c;
    else return __dadd_rn(a, kb) <= c && __dadd_rn(b, ka) <= c;
}

// the j of rows [0, rows) of the staged chunk against the register tile; DIAG: the chunk lies in tile I, count i < j only
template <int FORM, bool DIAG>
__device__ __forceinline__ void ln_chunk(const double (*Bs)[LN_LDB], const double (*Cs)[LN_COLS], int rows, int x, int y, int jrel,
                                         double kappa, const double (&a)[LN_R][LN_C], const double (&ka)[LN_R][LN_C],
                                         u32 (&cnt)[LN_R]) {
#pragma unroll 2
    for (int k = 0; k < rows; ++k) {
        double b[LN_R], kb[LN_R], c[LN_C];
#pragma unroll
        for (int r = 0; r < LN_R; r += 2) {
            const double2 v = *reinterpret_cast<const double2 *>(&Bs[k][LN_R * y + r]);
            b[r] = v.x, b[r + 1] = v.y;
        }
#pragma unroll
        for (int r = 0; r < LN_R; ++r) kb[r] = FORM == LN_GENERAL ? __dmul_rn(kappa, b[r]) : 0.0;
#pragma unroll
        for (int cc = 0; cc < LN_C / 2; ++cc) {
            const double2 v = *reinterpret_cast<const double2 *>(&Cs[k][32 * cc + 2 * x]);
            c[2 * cc] = v.x, c[2 * cc + 1] = v.y;
        }
#pragma unroll
        for (int cc = 0; cc < LN_C; ++cc) {
            const bool upper = !DIAG || 32 * (cc >> 1) + 2 * x + (cc & 1) < jrel + k;   // i < j, both relative to the tile
#pragma unroll
            for (int r = 0; r < LN_R; ++r) cnt[r] += (ln_in<FORM>(a[r][cc], ka[r][cc], b[r], kb[r], c[cc]) && upper) ? 1u : 0u;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// blockIdx.x = (tb * nt + I) * ng + g: the targets [q_first + 128 tb ...), the sample curves i of tile I, the tiles J of span g,
// [max(I, g span), min(nt, (g + 1) span)).  D: the n x n matrix.  R, targets, row0: the targets' rows, row q at
// R + (targets ? targets[q] : q - row0) * n.  q_end: one past the last target.  out[q] += the count.
template <int FORM>
__global__ __launch_bounds__(LN_THREADS, 2) void lens_count_kernel(const double *__restrict__ D, i64 n, const double *__restrict__ R,
                                                                const i64 *__restrict__ targets, i64 row0, i64 q_first, i64 q_end,
                                                                i64 nt, i64 ng, i64 span, double kappa,
                                                                unsigned long long *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) double Bs[LN_JK][LN_LDB];
    __shared__ __attribute__((aligned(16))) double Cs[LN_JK][LN_COLS];
    __shared__ i64 rowoff[LN_TILE];
    const int tid = threadIdx.x, x = tid & 15, y = tid >> 4;
    const i64 g = (i64)blockIdx.x % ng, I = (i64)blockIdx.x / ng % nt, tb = (i64)blockIdx.x / ng / nt;
    i64 Jb = g * span, Je = Jb + span;
    Jb = Jb < I ? I : Jb;
    Je = Je < nt ? Je : nt;
    if (Jb >= Je) return;                                           // the span lies below the diagonal
    const i64 q0 = q_first + tb * LN_TILE, i0 = I * LN_COLS;

    if (tid < LN_TILE) {
        const i64 q = q0 + tid;
        rowoff[tid] = q < q_end ? (targets ? targets[q] : q - row0) * n : -1;
    }
    __syncthreads();

    // the register tile: a = D2(target, curve i), +inf where either does not exist
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double a[LN_R][LN_C], ka[LN_R][LN_C];
    u32 cnt[LN_R];
#pragma unroll
    for (int r = 0; r < LN_R; ++r) {
        const i64 off = rowoff[LN_R * y + r];
        cnt[r] = 0;
#pragma unroll
        for (int c = 0; c < LN_C; ++c) {
            const i64 i = i0 + 32 * (c >> 1) + 2 * x + (c & 1);
            a[r][c] = off >= 0 && i < n ? R[off + i] : inf;
            ka[r][c] = FORM == LN_GENERAL ? __dmul_rn(kappa, a[r][c]) : 0.0;
        }
    }

    // a thread fetches of the matrix one column i at the rows (tid >> 6) + 4 l of a chunk, and of the targets' panel the row
    // tid & 15 for the targets (tid >> 4) + 16 l
    const int col = tid & (LN_COLS - 1), kc0 = tid >> 6;
    const i64 jend = Je * LN_COLS < n ? Je * LN_COLS : n;
    for (i64 j0 = Jb * LN_COLS; j0 < jend; j0 += LN_JK) {
        __syncthreads();                                            // the chunk before is consumed
#pragma unroll
        for (int l = 0; l < LN_JK / 4; ++l) {
            const i64 j = j0 + kc0 + 4 * l, i = i0 + col;
            Cs[kc0 + 4 * l][col] = j < n && i < n ? D[j * n + i] : 0.0;
        }
#pragma unroll
        for (int l = 0; l < LN_TILE / 16; ++l) {
            const i64 off = rowoff[y + 16 * l], j = j0 + x;
            Bs[x][y + 16 * l] = off >= 0 && j < n ? R[off + j] : 0.0;
        }
        __syncthreads();
        const int rows = jend - j0 < LN_JK ? (int)(jend - j0) : LN_JK;
        if (j0 < i0 + LN_COLS) ln_chunk<FORM, true>(Bs, Cs, rows, x, y, (int)(j0 - i0), kappa, a, ka, cnt);
        else ln_chunk<FORM, false>(Bs, Cs, rows, x, y, 0, kappa, a, ka, cnt);
    }

#pragma unroll
    for (int r = 0; r < LN_R; ++r) {
        u32 v = cnt[r];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        v += __shfl_xor(v, 8);
        const i64 q = q0 + LN_R * y + r;
        if (x == 0 && q < q_end && v) atomicAdd(&out[q], (unsigned long long)v);
    }
}

// ---------------------------------------------------------------------------------------------- the batch plan
LensPlan lens_plan(i64 n, i64 m, PlanSize size) {
    LensPlan p{0, 0, 0, 0};
    p.matrix = align_up((size_t)n * (size_t)n * 8, 256);
    const size_t rb = (size_t)LN_TILE * (size_t)n * 8;              // the rows of 128 external targets; a multiple of 256
    const TargetBlocks b = target_block_plan(m, size, rb, rb, LN_ROWS_MAX, p.matrix);   // bytes below the matrix: no block
    if (b.blocks < 1) return p;
    p.targets = b.targets;
    p.rows = (size_t)b.blocks * rb;
    p.bytes = p.matrix + p.rows;
    return p;
}

i64 lens_span(i64 n, i64 targets) {
    const i64 nt = ln_tiles(n), tb = (targets + LN_TILE - 1) / LN_TILE;
    i64 span = tb * nt * nt / LN_GROUPS_WANTED;
    span = span < 1 ? 1 : span;
    return span < nt ? span : nt;
}

// ---------------------------------------------------------------------------------------------- host
// the counts of the targets [q_begin, q_end) into out (zeroed by the caller), nt * ng workgroups a target block
template <int FORM>
static int ln_launch(const double *D, i64 n, const double *R, const i64 *targets, i64 q_begin, i64 q_end, double kappa, i64 *out,
                     hipStream_t s) {
    const i64 nt = ln_tiles(n), span = lens_span(n, q_end - q_begin), ng = (nt + span - 1) / span;
    return for_block_launches(q_begin, q_end, nt * ng, [&](i64 q, i64 tb) -> int {
        hipLaunchKernelGGL(lens_count_kernel<FORM>, dim3((unsigned)(tb * nt * ng)), dim3(LN_THREADS), 0, s, D, n, R, targets, q_begin, q,
                           q_end, nt, ng, span, kappa, (unsigned long long *)out);
        SD_HIP(hipGetLastError());
        return SD_OK;
    });
}

static int ln_launch_form(int form, const double *D, i64 n, const double *R, const i64 *targets, i64 q_begin, i64 q_end, double kappa,
                          i64 *out, hipStream_t s) {
    if (form == LN_LENS) return ln_launch<LN_LENS>(D, n, R, targets, q_begin, q_end, kappa, out, s);
    if (form == LN_SPHERE) return ln_launch<LN_SPHERE>(D, n, R, targets, q_begin, q_end, kappa, out, s);
    return ln_launch<LN_GENERAL>(D, n, R, targets, q_begin, q_end, kappa, out, s);
}

int lens_form(double kappa, int algo) { return algo == 1 ? LN_GENERAL : kappa == 0.0 ? LN_LENS : kappa == 1.0 ? LN_SPHERE : LN_GENERAL; }

int launch_lens_counts(const double *Y, i64 T, i64 n, CurveSel sel, i64 m, double kappa, int algo, i64 *out, void *ws, size_t ws_bytes,
                       hipStream_t s) {
    const LensPlan plan = lens_plan(n, m, PlanSize::of_bytes(ws_bytes));
    Carver cv(ws, ws_bytes);
    double *D = plan.targets > 0 ? (double *)cv.take(plan.matrix) : nullptr;
    double *A = D ? (double *)cv.take(plan.rows) : nullptr;
    if (!D || !A) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_lens_min_workspace_bytes)");
    const int form = lens_form(kappa, algo);
    int rc = launch_curve_sqdist(Y, T, n, select_sample(nullptr), n, D, s);
    if (rc) return rc;
    SD_HIP(hipMemsetAsync(out, 0, (size_t)m * 8, s));
    if (!sel.Q) return ln_launch_form(form, D, n, D, sel.targets, 0, m, kappa, out, s);   // targets null: all in order, row q of D
    return for_target_batches(m, plan.targets, [&](i64 q, i64 count) -> int {
        const int rc = launch_curve_sqdist_rows(Y, T, n, sel.Q, m, q, q + count, A, s);
        return rc ? rc : ln_launch_form(form, D, n, A, nullptr, q, q + count, kappa, out, s);
    });
}

}  // namespace sd
