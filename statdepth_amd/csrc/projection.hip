// projection.hip -- K12: projection depth (Stahel-Donoho outlyingness) of a point cloud over a fixed set of directions.
//
// Definition.  A sample S of N points in R^d, d <= 8, directions u_0 .. u_(k-1) (rows of a k x d fp64 array), a target q:
//   z_r(x)    = K10's projection, the same bits (hs_proj: features in increasing order, every product and every sum rounded
//               separately to fp64, no FMA);
//   median(v) of N values sorted ascending as s: s[(N-1)/2] for N odd, (s[N/2-1] + s[N/2]) * 0.5 for N even (the sum
//               rounded, then the product rounded);
//   med_r     = median(z_r(S));   dev_i = |z_r(p_i) - med_r| (one rounded subtraction, the sign cleared);
//   mad_r     = median(dev), the same rule, no 1.4826 factor;
//   o_r(q)    = |z_r(q) - med_r| / mad_r, one correctly rounded division; a numerator of 0 gives 0 whatever mad_r is, a
//               numerator above 0 with mad_r = 0 gives +inf;
//   O(q)      = max over r of o_r(q);   depth = 1 / (1 + O) on the host (O = inf: 0.0).
// Every step is one correctly rounded fp64 operation (__dsub_rn, __dadd_rn, __dmul_rn, __ddiv_rn) or an order statistic,
// so a numpy restatement gives the same bits.  No NaN arises: the data and the directions are finite, with magnitudes of
// at most 2^500 so that no projection or midpoint overflows (the Python layer refuses anything else).
// The sample per form (point_select.h): rows -- all n rows, the target among them; external -- P u {Q[q]}, N = n + 1,
// every external point with a median and a MAD of its own; blocks -- the block's members, the target last; an empty
// block yields 0.
//
// Selection (pd_locscale, in projection_select.h: K18 uses it too): from a sorted sequence s of length N, med by the rule above, then the MAD WITHOUT sorting the
// deviations.  With a = lower_bound(s, med), med - s[a-1-j] (j = 0 .. a-1) and s[a+j] - med (j = 0 .. N-a-1) are two
// ascending sequences (rounding is monotone, so the rounded deviations keep their order); the floor((N-1)/2)-th smallest
// of their union comes from a merge-path binary search, the floor(N/2)-th is the next of the merge.  O(log N) reads.
// Three accessors: a sorted global row, such a row with one value virtually inserted at its lower_bound position
// (external form), a sorted LDS array (blocks form).
//
// Rows and external forms, per chunk of kc directions (the chunk of K10's ranking route, launch_hs_sort_chunk):
//   projection + tile sort + merge passes leave every direction's projections sorted in the workspace;
//   rows:     pd_locscale_kernel writes med[r], mad[r] of the chunk (a wave per direction: its 64 lanes probe 64 positions
//             per round of a search, 4 dependent reads for 10^6 values where a thread's binary search has 20);
//             pd_outlyingness_kernel: a thread owns a target, recomputes its projection per direction (wave-uniform
//             direction loads), keeps the running maximum in a register and folds it into out[q].  Chunks are
//             stream-ordered, so the fold is a plain read-modify-write;
//   external: pd_external_kernel, a thread per (external point, direction of the chunk): selection through the
//             inserted-value accessor, then atomicMax on the 64-bit pattern into the zeroed out[] (non-negative doubles
//             order like their bit patterns, +inf above all of them).
//   The maximum is exact and order-free, so the result does not depend on kc, i.e. on the workspace size.
// Blocks form: pd_blocks_kernel, one workgroup of 256 threads per block of at most PD_MAX_BLOCK = 2048 members; per direction
//   the members' projections go to LDS (16 KB of keys), padded with +inf to the next power of two, a bitonic network
//   sorts them, thread 0 selects and evaluates the target.  A launch covers at most PD_UNITS blocks and PD_BLOCK_DIRS
//   directions; out[q] is written once per launch (folded across the direction launches in stream order).
//
// LDS budget: blocks form 16 KB of keys + the member count; the other kernels of this file use none (the shared sort: 24
// KB per tile, 48 KB per merge).  256 threads per workgroup (64 for pd_locscale_kernel).  Every launch is bounded: a
// chunk covers at most max(n, 2^25) values, pd_external_kernel at most PD_UNITS workgroups, pd_blocks_kernel at most
// PD_UNITS x PD_BLOCK_DIRS sorts of 2048 keys.  No kernel waits on another workgroup.
#include "sd_common.h"
#include "point_select.h"
#include "halfspace_sort.h"
#include "projection_select.h"

namespace sd {

constexpr int PD_THREADS = 256;
constexpr int PD_LOC_THREADS = 64;                                 // pd_locscale_kernel: one wave64 per direction
constexpr u64 PD_UNITS = (u64)1 << 14;                             // workgroups per launch (external, blocks)
constexpr i64 PD_BLOCK_DIRS = 256;                                 // blocks form: directions per launch
static_assert((PD_MAX_BLOCK & (PD_MAX_BLOCK - 1)) == 0, "the bitonic network pads a block to a power of two inside sk[]");

// ---------------------------------------------------------------------------------------------- rows form
// a wave per direction of the chunk (one wave64 per workgroup, PdWaveSearch): K is kk x n, every row sorted
__global__ __launch_bounds__(PD_LOC_THREADS) void pd_locscale_kernel(const double *__restrict__ K, i64 n,
                                                                     double *__restrict__ med, double *__restrict__ mad) {
    const i64 r = blockIdx.x;
    double a, b;
    pd_locscale(PdGlobalRow{K + r * n}, n, a, b, PdWaveSearch());
    if (threadIdx.x == 0) {
        med[r] = a;
        mad[r] = b;
    }
}

// a thread per target: out[j] = max(out[j], max over the chunk's directions of o_r); first: the chunk starts the maximum
template <int D>
__global__ __launch_bounds__(PD_THREADS) void pd_outlyingness_kernel(const double *__restrict__ P,
                                                                     const double *__restrict__ U, int kk,
                                                                     const double *__restrict__ med,
                                                                     const double *__restrict__ mad,
                                                                     const i64 *__restrict__ targets, i64 m, int first,
                                                                     double *__restrict__ out) {
    const i64 j = (i64)blockIdx.x * PD_THREADS + threadIdx.x;
    if (j >= m) return;
    const i64 row = targets ? targets[j] : j;
    double x[D];
#pragma unroll
    for (int e = 0; e < D; ++e) x[e] = P[row * D + e];
    double best = first ? 0.0 : out[j];
    for (int r = 0; r < kk; ++r) {
        double u[D];
#pragma unroll
        for (int e = 0; e < D; ++e) u[e] = U[(i64)r * D + e];      // wave-uniform
        const double o = pd_outlyingness(hs_proj<D>(x, u), med[r], mad[r]);
        best = o > best ? o : best;
    }
    out[j] = best;
}

// ---------------------------------------------------------------------------------------------- external form
// a thread per (external point q, direction r of the chunk), g = r * m + q; out zeroed before the first chunk
template <int D>
__global__ __launch_bounds__(PD_THREADS) void pd_external_kernel(const double *__restrict__ K, i64 n,
                                                                 const double *__restrict__ U, int kk,
                                                                 const double *__restrict__ Q, i64 m, i64 g0, i64 total,
                                                                 u64 *__restrict__ out) {
    const i64 g = g0 + (i64)blockIdx.x * PD_THREADS + threadIdx.x;
    if (g >= total) return;
    const i64 r = g / m, q = g % m;
    double x[D], u[D];
#pragma unroll
    for (int e = 0; e < D; ++e) {
        x[e] = Q[q * D + e];
        u[e] = U[r * D + e];
    }
    const double z = hs_proj<D>(x, u);
    const double *row = K + r * n;
    const PdInsertedRow s{row, pd_lower_bound(PdGlobalRow{row}, n, z), z};
    double med, mad;
    pd_locscale(s, n + 1, med, mad);
    const double o = pd_outlyingness(z, med, mad);
    if (o > 0.0) atomicMax(&out[q], (u64)__double_as_longlong(o));
}

// ---------------------------------------------------------------------------------------------- blocks form
// one workgroup per block q0 + blockIdx.x, directions [r0, r1)
template <int D>
__global__ __launch_bounds__(PD_THREADS) void pd_blocks_kernel(const double *__restrict__ P, i64 n,
                                                               const double *__restrict__ U, i64 r0, i64 r1, PointSel sel,
                                                               i64 q0, double *__restrict__ out) {
    __shared__ double sk[PD_MAX_BLOCK];
    __shared__ int s_cnt;
    const i64 q = q0 + blockIdx.x;
    const PointView v = point_view_coop<PD_THREADS>(sel, P, n, D, q, &s_cnt);
    const int cnt = (int)v.cnt;
    if (cnt == 0) {                                                 // (block-uniform) an empty block
        if (threadIdx.x == 0) out[q] = 0.0;
        return;
    }
    int N2 = 1;
    while (N2 < cnt) N2 <<= 1;
    double xt[D];
#pragma unroll
    for (int e = 0; e < D; ++e) xt[e] = v.x[e];
    double best = r0 == 0 ? 0.0 : out[q];                           // used by thread 0 alone
    for (i64 r = r0; r < r1; ++r) {
        double u[D];
#pragma unroll
        for (int e = 0; e < D; ++e) u[e] = U[r * D + e];           // wave-uniform
        for (int p = threadIdx.x; p < N2; p += PD_THREADS) {
            double z = __longlong_as_double(0x7ff0000000000000LL);
            if (p < cnt) {
                const double *xp = P + (i64)v.mem[p] * D;
                double x[D];
#pragma unroll
                for (int e = 0; e < D; ++e) x[e] = xp[e];
                z = hs_proj<D>(x, u);
            }
            sk[p] = z;
        }
        __syncthreads();
        for (int k = 2; k <= N2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int x = threadIdx.x; x < (N2 >> 1); x += PD_THREADS) {
                    const int i = ((x & ~(j - 1)) << 1) | (x & (j - 1));
                    const int l = i | j;
                    const bool up = (i & k) == 0;
                    const double a = sk[i], b = sk[l];
                    if ((a > b) == up) {
                        sk[i] = b;
                        sk[l] = a;
                    }
                }
                __syncthreads();
            }
        }
        if (threadIdx.x == 0) {
            double med, mad;
            pd_locscale(PdLdsRow{sk}, cnt, med, mad);
            const double o = pd_outlyingness(hs_proj<D>(xt, u), med, mad);
            best = o > best ? o : best;
        }
        __syncthreads();                                            // the selection has read sk before the next projection
    }
    if (threadIdx.x == 0) out[q] = best;
}

// ---------------------------------------------------------------------------------------------- launchers
// fixed part (the alignment of the seven carve-outs) and the part per direction of a chunk (sort buffers, med, mad)
static inline size_t pd_ws_fixed() { return (size_t)(HS_SORT_CARVES + 2) * 256; }
static inline size_t pd_ws_per_direction(i64 n) { return hs_sort_bytes_per_direction(n) + 16; }

int launch_pd_locscale(const double *K, i64 n, int kk, double *med, double *mad, hipStream_t s) {
    hipLaunchKernelGGL(pd_locscale_kernel, dim3((unsigned)kk), dim3(PD_LOC_THREADS), 0, s, K, n, med, mad);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

size_t projection_min_workspace_bytes(i64 n) { return pd_ws_fixed() + pd_ws_per_direction(n); }

size_t projection_workspace_bytes(i64 n, i64 k) {
    i64 kc = HS_REC_VALUES / n;
    kc = kc < 1 ? 1 : kc > k ? k : kc;
    return pd_ws_fixed() + (size_t)kc * pd_ws_per_direction(n);
}

template <int D>
static int launch_pd_sorted_d(const double *P, i64 n, const double *U, i64 k, const PointSel &sel, i64 m, double *out,
                              void *ws, size_t ws_bytes, hipStream_t s) {
    if (!ws || ws_bytes < projection_min_workspace_bytes(n))
        return fail(SD_ERR_WORKSPACE, "workspace too small for one direction per chunk (sd_projection_min_workspace_bytes)");
    const i64 kc = hs_chunk_directions(ws_bytes - pd_ws_fixed(), pd_ws_per_direction(n), n, k);
    Carver cv(ws, ws_bytes);
    HsSortBuffers b;
    const bool carved = hs_sort_carve(cv, n, kc, b);
    double *med = (double *)cv.take((size_t)kc * 8);
    double *mad = (double *)cv.take((size_t)kc * 8);
    if (!carved || !med || !mad) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_projection_min_workspace_bytes)");
    if (sel.Q) SD_HIP(hipMemsetAsync(out, 0, (size_t)m * 8, s));
    for (i64 c0 = 0; c0 < k; c0 += kc) {
        const int kk = (int)(k - c0 < kc ? k - c0 : kc);
        const double *Uc = U + c0 * D;
        int src = 0;
        const int rc = launch_hs_sort_chunk(P, n, D, Uc, kk, b, &src, s);
        if (rc) return rc;
        if (sel.Q) {
            const i64 total = (i64)kk * m;
            const i64 per = (i64)PD_UNITS * PD_THREADS;
            for (i64 g0 = 0; g0 < total; g0 += per) {
                const i64 cnt = total - g0 < per ? total - g0 : per;
                hipLaunchKernelGGL((pd_external_kernel<D>), dim3((unsigned)((cnt + PD_THREADS - 1) / PD_THREADS)),
                                   dim3(PD_THREADS), 0, s, b.K[src], n, Uc, kk, sel.Q, m, g0, total, (u64 *)out);
                SD_HIP(hipGetLastError());
            }
        } else {
            if (const int rl = launch_pd_locscale(b.K[src], n, kk, med, mad, s)) return rl;
            hipLaunchKernelGGL((pd_outlyingness_kernel<D>), dim3((unsigned)((m + PD_THREADS - 1) / PD_THREADS)),
                               dim3(PD_THREADS), 0, s, P, Uc, kk, med, mad, sel.targets, m, c0 == 0 ? 1 : 0, out);
            SD_HIP(hipGetLastError());
        }
    }
    return SD_OK;
}

template <int D>
static int launch_pd_blocks_d(const double *P, i64 n, const double *U, i64 k, const PointSel &sel, i64 nb, double *out,
                              hipStream_t s) {
    for (i64 q0 = 0; q0 < nb; q0 += (i64)PD_UNITS) {
        const i64 g = nb - q0 < (i64)PD_UNITS ? nb - q0 : (i64)PD_UNITS;
        for (i64 r0 = 0; r0 < k; r0 += PD_BLOCK_DIRS) {
            const i64 r1 = r0 + PD_BLOCK_DIRS < k ? r0 + PD_BLOCK_DIRS : k;
            hipLaunchKernelGGL((pd_blocks_kernel<D>), dim3((unsigned)g), dim3(PD_THREADS), 0, s, P, n, U, r0, r1, sel, q0, out);
            SD_HIP(hipGetLastError());
        }
    }
    return SD_OK;
}

int launch_projection_sorted(const double *P, i64 n, int d, const double *U, i64 k, const PointSel &sel, i64 m, double *out,
                             void *ws, size_t ws_bytes, hipStream_t s) {
    SD_DISPATCH_D(d, return launch_pd_sorted_d<D_>(P, n, U, k, sel, m, out, ws, ws_bytes, s))
    return fail(SD_ERR_UNSUPPORTED, "projection outlyingness covers d in [1,8], got %d", d);
}

int launch_projection_blocks(const double *P, i64 n, int d, const double *U, i64 k, const PointSel &sel, i64 nb, double *out,
                             hipStream_t s) {
    SD_DISPATCH_D(d, return launch_pd_blocks_d<D_>(P, n, U, k, sel, nb, out, s))
    return fail(SD_ERR_UNSUPPORTED, "projection outlyingness covers d in [1,8], got %d", d);
}

}  // namespace sd
