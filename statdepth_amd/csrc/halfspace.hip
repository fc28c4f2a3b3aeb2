// halfspace.hip -- K10: halfspace (Tukey) depth of a point cloud over a fixed set of directions.
//
// Definition.  Points p_0 .. p_(n-1) in R^d, directions u_0 .. u_(k-1) (rows of a k x d fp64 array), a target q:
//   z_r(x)  = ((x_0 u_r0 + x_1 u_r1) + x_2 u_r2) + ...   features in increasing order, every product and every sum rounded
//             separately to fp64 (__dmul_rn / __dadd_rn, no FMA), so a numpy loop over the features gives the same bits;
//   ge_r(q) = #{i : z_r(p_i) >= z_r(q)},  le_r(q) = #{i : z_r(p_i) <= z_r(q)}   (q itself and every tie counted);
//   count(q) = min over r of min(ge_r(q), le_r(q))   (one direction serves u and -u),   depth = count / n.
// An external target g is counted inside F u {g}: n + 1 points, g counted once, depth = count / (n + 1).
// This is the directional ("random Tukey", Cuesta-Albertos & Nieto-Reyes) depth: for d >= 2 an upper bound of the exact
// halfspace depth, which is the infimum over all directions; with d = 1 and the direction (1.0) it is exact.
// Projections must be comparable (no NaN; the Python layer refuses non-finite data and directions).
//
// Two routes, the same projections bit for bit in both:
//
// Ranking route (sd_halfspace_counts, every sample point ranked whatever m is), per chunk of kc directions:
//   hs_project_kernel    Z[r][i] = z_r(p_i), a kc x n fp64 matrix in the workspace;
//   hs_tile_sort_kernel  each tile of HS_TILE = 2048 consecutive values of a row is sorted in LDS with the point's index
//                        as payload (bitonic network on (key, index); a tile shorter than 2048 runs the network of the
//                        next power of two);
//   hs_partition_kernel / hs_merge_kernel   log2(n / 2048) merge passes between two buffers: per output tile a
//                        merge-path split found by binary search in global memory, then both input runs (2048 values
//                        together) in LDS, every value placed by one binary search in the other run, output staged in
//                        LDS and written coalesced;
//   hs_rank_kernel       position p of the sorted row has lt = p and le = p + 1 unless a neighbour is equal (then a binary
//                        search finds the end of the run of ties); atomicMin(cnt[index], min(le, n - lt)).
//   After the last chunk hs_gather_kernel writes cnt[targets[j]] to out[j].  O(k n log n) comparisons, no all-pairs
//   pass.  Integer min is exact and order-free, so the counts do not depend on kc, i.e. on the workspace size.
//
// Pairwise route (sd_halfspace_external_counts, sd_halfspace_subset_counts): hs_pairwise_kernel, one workgroup per
// (target, 256 directions, slice of HS_SLICE sample points): a thread owns a direction (its u and the target's
// projection in registers), the slice passes through LDS in tiles of 256 points read by every lane at the same address
// (broadcast), projections recomputed in registers.  Slice counts are added with integer atomics (exact, order-free) into
// acc[target][direction][le, ge]; hs_reduce_kernel takes the minimum over the directions.
//
// LDS budget: tile sort 24 KB (2048 x (8 + 4) bytes), merge 48 KB (input and output images), pairwise 256 x d x 8 bytes
// (16 KB at d = 8).  256 threads (4 wave64) per workgroup everywhere.  Every launch is bounded: a ranking launch covers at
// most max(n, 2^25) values, a pairwise launch at most HS_UNITS workgroups of HS_SLICE x 256 projections each.
//
// The projection and the sorted rows (hs_proj, launch_hs_sort_chunk) are shared with K12 (projection.hip) through
// halfspace_sort.h; the sort without the projection (launch_hs_sort_rows) serves K14's rows of curves (rank_depths.hip).
#include "sd_common.h"
#include "point_select.h"
#include "halfspace_sort.h"

namespace sd {

constexpr int HS_PTILE = 256;                                      // pairwise: sample points per LDS tile
constexpr i64 HS_SLICE = 4096;                                     // pairwise: sample points per workgroup
constexpr u64 HS_UNITS = (u64)1 << 14;                             // pairwise: workgroups per launch
constexpr size_t HS_ACC_BYTES = (size_t)64 << 20;                  // pairwise: accumulator bytes per batch of targets

// ---------------------------------------------------------------------------------------------- ranking route
template <int D>
__global__ __launch_bounds__(HS_THREADS) void hs_project_kernel(const double *__restrict__ P, i64 n,
                                                                const double *__restrict__ U, int kc,
                                                                double *__restrict__ Z) {
    const i64 i = (i64)blockIdx.x * HS_THREADS + threadIdx.x;
    if (i >= n) return;
    double x[D];
#pragma unroll
    for (int e = 0; e < D; ++e) x[e] = P[i * D + e];
    for (int r = blockIdx.y; r < kc; r += gridDim.y) {
        double u[D];
#pragma unroll
        for (int e = 0; e < D; ++e) u[e] = U[(i64)r * D + e];      // wave-uniform
        Z[(i64)r * n + i] = hs_proj<D>(x, u);
    }
}

// one workgroup per (row, tile): K (in place) sorted ascending inside the tile, I = the values' columns
__global__ __launch_bounds__(HS_THREADS) void hs_tile_sort_kernel(double *__restrict__ K, u32 *__restrict__ I, i64 n,
                                                                  int ntiles) {
    __shared__ double sk[HS_TILE];
    __shared__ u32 si[HS_TILE];
    const i64 r = blockIdx.x / ntiles;
    const int t = blockIdx.x % ntiles;
    const i64 base = (i64)t * HS_TILE;
    const int cnt = (int)(n - base < HS_TILE ? n - base : HS_TILE);
    int N2 = 2;
    while (N2 < cnt) N2 <<= 1;
    double *Kr = K + r * n + base;
    u32 *Ir = I + r * n + base;
    for (int p = threadIdx.x; p < N2; p += HS_THREADS) {
        sk[p] = p < cnt ? Kr[p] : __longlong_as_double(0x7ff0000000000000LL);
        si[p] = p < cnt ? (u32)(base + p) : 0xffffffffu;          // a padding slot sorts behind every real +inf
    }
    __syncthreads();
    for (int k = 2; k <= N2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = threadIdx.x; x < (N2 >> 1); x += HS_THREADS) {
                const int i = ((x & ~(j - 1)) << 1) | (x & (j - 1));
                const int l = i | j;
                const bool up = (i & k) == 0;
                const double a = sk[i], b = sk[l];
                const u32 ia = si[i], ib = si[l];
                const bool gt = a > b || (a == b && ia > ib);
                if (gt == up) {
                    sk[i] = b; sk[l] = a;
                    si[i] = ib; si[l] = ia;
                }
            }
            __syncthreads();
        }
    }
    for (int p = threadIdx.x; p < cnt; p += HS_THREADS) {
        Kr[p] = sk[p];
        Ir[p] = si[p];
    }
}

// the runs a merge pass of width w joins, seen from output tile t of a row
struct HsPair {
    i64 pb;                                                         // first column of the pair
    int lenL, lenR, d0;                                             // run lengths, the tile's first output inside the pair
};

__device__ __forceinline__ HsPair hs_pair(i64 n, i64 w, int t) {
    HsPair p;
    const i64 o = (i64)t * HS_TILE;
    p.pb = o / (2 * w) * (2 * w);
    const i64 left = n - p.pb;
    p.lenL = (int)(left < w ? left : w);
    p.lenR = (int)(left - p.lenL < w ? left - p.lenL : w);
    p.d0 = (int)(o - p.pb);
    return p;
}

// part[row][t] = how many of the first d0 outputs of tile t's pair come from the left run (ties: left first)
__global__ __launch_bounds__(HS_THREADS) void hs_partition_kernel(const double *__restrict__ K, i64 n, i64 w, int ntiles,
                                                                  i64 total, int *__restrict__ part) {
    const i64 g = (i64)blockIdx.x * HS_THREADS + threadIdx.x;
    if (g >= total) return;
    const i64 r = g / ntiles;
    const int t = (int)(g % ntiles);
    const HsPair p = hs_pair(n, w, t);
    const double *L = K + r * n + p.pb;
    const double *R = L + p.lenL;
    int lo = p.d0 > p.lenR ? p.d0 - p.lenR : 0;
    int hi = p.d0 < p.lenL ? p.d0 : p.lenL;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (L[mid] <= R[p.d0 - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    part[g] = lo;
}

// one workgroup per (row, output tile)
__global__ __launch_bounds__(HS_THREADS) void hs_merge_kernel(const double *__restrict__ Ks, const u32 *__restrict__ Is,
                                                              double *__restrict__ Kd, u32 *__restrict__ Id, i64 n, i64 w,
                                                              int ntiles, const int *__restrict__ part) {
    __shared__ double sk[HS_TILE];
    __shared__ double ok[HS_TILE];
    __shared__ u32 si[HS_TILE];
    __shared__ u32 oi[HS_TILE];
    const i64 r = blockIdx.x / ntiles;
    const int t = blockIdx.x % ntiles;
    const HsPair p = hs_pair(n, w, t);
    const int len = p.lenL + p.lenR;
    const int d1 = (i64)p.d0 + HS_TILE < len ? p.d0 + HS_TILE : len;
    const int a0 = part[blockIdx.x];
    const int a1 = d1 == len ? p.lenL : part[blockIdx.x + 1];      // d1 < len: tile t + 1 lies in the same pair
    const int b0 = p.d0 - a0, b1 = d1 - a1;
    const int na = a1 - a0, nb = b1 - b0, cnt = na + nb;
    const i64 row = r * n + p.pb;
    for (int x = threadIdx.x; x < cnt; x += HS_THREADS) {
        const i64 src = row + (x < na ? a0 + x : p.lenL + b0 + (x - na));
        sk[x] = Ks[src];
        si[x] = Is[src];
    }
    __syncthreads();
    for (int x = threadIdx.x; x < cnt; x += HS_THREADS) {
        const double key = sk[x];
        int pos;
        if (x < na) {                                               // + the values of the right run below key
            int lo = 0, hi = nb;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sk[na + mid] < key) lo = mid + 1;
                else hi = mid;
            }
            pos = x + lo;
        } else {                                                    // + the values of the left run not above key
            int lo = 0, hi = na;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sk[mid] <= key) lo = mid + 1;
                else hi = mid;
            }
            pos = x - na + lo;
        }
        ok[pos] = key;
        oi[pos] = si[x];
    }
    __syncthreads();
    const i64 dst = row + p.d0;
    for (int x = threadIdx.x; x < cnt; x += HS_THREADS) {
        Kd[dst + x] = ok[x];
        Id[dst + x] = oi[x];
    }
}

// sorted rows -> cnt[column] = min(cnt[column], min(le, ge))
__global__ __launch_bounds__(HS_THREADS) void hs_rank_kernel(const double *__restrict__ K, const u32 *__restrict__ I, i64 n,
                                                             i64 total, u32 *__restrict__ cnt) {
    const i64 g = (i64)blockIdx.x * HS_THREADS + threadIdx.x;
    if (g >= total) return;
    const i64 r = g / n, p = g % n;
    const double *Kr = K + r * n;
    const double key = Kr[p];
    i64 lt = p, le = p + 1;
    if (p > 0 && Kr[p - 1] == key) {                                // first position of the run of ties
        i64 lo = 0, hi = p;
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if (Kr[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        lt = lo;
    }
    if (p + 1 < n && Kr[p + 1] == key) {                            // one past its last position
        i64 lo = p + 1, hi = n;
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if (Kr[mid] <= key) lo = mid + 1;
            else hi = mid;
        }
        le = lo;
    }
    const i64 ge = n - lt;
    const u32 col = I[g];
    if (col < n) atomicMin(&cnt[col], (u32)(le < ge ? le : ge));   // (a padding index can surface only among NaN keys)
}

__global__ __launch_bounds__(HS_THREADS) void hs_gather_kernel(const u32 *__restrict__ cnt, const i64 *__restrict__ targets,
                                                               i64 m, i64 *__restrict__ out) {
    const i64 j = (i64)blockIdx.x * HS_THREADS + threadIdx.x;
    if (j >= m) return;
    out[j] = (i64)cnt[targets ? targets[j] : j];
}

// fixed part (the running minima and the alignment of the six carve-outs) and the part per direction of a chunk
static inline size_t hs_ws_fixed(i64 n) { return align_up((size_t)n * 4, 256) + (1 + HS_SORT_CARVES) * 256; }
static inline size_t hs_ws_per_direction(i64 n) { return hs_sort_bytes_per_direction(n); }

size_t halfspace_min_workspace_bytes(i64 n) { return hs_ws_fixed(n) + hs_ws_per_direction(n); }

size_t halfspace_workspace_bytes(i64 n, i64 k) {
    i64 kc = HS_REC_VALUES / n;
    kc = kc < 1 ? 1 : kc > k ? k : kc;
    return hs_ws_fixed(n) + (size_t)kc * hs_ws_per_direction(n);
}

// kk rows of n values already in b.K[0]: tile sort, merge passes; the sorted rows are in b.K[*src] / b.I[*src]
int launch_hs_sort_rows(i64 n, int kk, const HsSortBuffers &b, int *src_out, hipStream_t s) {
    const int ntiles = hs_ntiles(n);
    const i64 tiles = (i64)kk * ntiles;
    hipLaunchKernelGGL(hs_tile_sort_kernel, dim3((unsigned)tiles), dim3(HS_THREADS), 0, s, b.K[0], b.I[0], n, ntiles);
    SD_HIP(hipGetLastError());
    int src = 0;
    for (i64 w = HS_TILE; w < n; w *= 2) {
        hipLaunchKernelGGL(hs_partition_kernel, dim3((unsigned)((tiles + HS_THREADS - 1) / HS_THREADS)), dim3(HS_THREADS),
                           0, s, b.K[src], n, w, ntiles, tiles, b.part);
        SD_HIP(hipGetLastError());
        hipLaunchKernelGGL(hs_merge_kernel, dim3((unsigned)tiles), dim3(HS_THREADS), 0, s, b.K[src], b.I[src], b.K[src ^ 1],
                           b.I[src ^ 1], n, w, ntiles, b.part);
        SD_HIP(hipGetLastError());
        src ^= 1;
    }
    *src_out = src;
    return SD_OK;
}

// one chunk: projection into b.K[0], then launch_hs_sort_rows
template <int D>
static int hs_sort_chunk_d(const double *P, i64 n, const double *U, int kk, const HsSortBuffers &b, int *src_out,
                           hipStream_t s) {
    const unsigned gx = (unsigned)((n + HS_THREADS - 1) / HS_THREADS);
    unsigned gy = gx >= 2048 ? 1 : (2048 + gx - 1) / gx;
    gy = gy > (unsigned)kk ? (unsigned)kk : gy;
    hipLaunchKernelGGL((hs_project_kernel<D>), dim3(gx, gy), dim3(HS_THREADS), 0, s, P, n, U, kk, b.K[0]);
    SD_HIP(hipGetLastError());
    return launch_hs_sort_rows(n, kk, b, src_out, s);
}

int launch_hs_sort_chunk(const double *P, i64 n, int d, const double *U, int kk, const HsSortBuffers &b, int *src,
                         hipStream_t s) {
    SD_DISPATCH_D(d, return hs_sort_chunk_d<D_>(P, n, U, kk, b, src, s))
    return fail(SD_ERR_UNSUPPORTED, "halfspace projections cover d in [1,8], got %d", d);
}

static int launch_hs_counts(const double *P, i64 n, int d, const double *U, i64 k, const i64 *targets, i64 m, i64 *out,
                            void *ws, size_t ws_bytes, hipStream_t s) {
    if (!ws || ws_bytes < halfspace_min_workspace_bytes(n))
        return fail(SD_ERR_WORKSPACE, "workspace too small for one direction per chunk (sd_halfspace_min_workspace_bytes)");
    const i64 kc = hs_chunk_directions(ws_bytes - hs_ws_fixed(n), hs_ws_per_direction(n), n, k);
    Carver cv(ws, ws_bytes);
    u32 *cnt = (u32 *)cv.take((size_t)n * 4);
    HsSortBuffers b;
    if (!hs_sort_carve(cv, n, kc, b) || !cnt)
        return fail(SD_ERR_WORKSPACE, "workspace too small (sd_halfspace_min_workspace_bytes)");
    SD_HIP(hipMemsetAsync(cnt, 0xff, (size_t)n * 4, s));
    for (i64 c0 = 0; c0 < k; c0 += kc) {
        const int kk = (int)(k - c0 < kc ? k - c0 : kc);
        int src = 0;
        const int rc = launch_hs_sort_chunk(P, n, d, U + c0 * d, kk, b, &src, s);
        if (rc) return rc;
        const i64 total = (i64)kk * n;
        hipLaunchKernelGGL(hs_rank_kernel, dim3((unsigned)((total + HS_THREADS - 1) / HS_THREADS)), dim3(HS_THREADS), 0, s,
                           b.K[src], b.I[src], n, total, cnt);
        SD_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(hs_gather_kernel, dim3((unsigned)((m + HS_THREADS - 1) / HS_THREADS)), dim3(HS_THREADS), 0, s, cnt,
                       targets, m, out);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------- pairwise route
// The targets are selected by a PointSel (point_select.h); the whole sample is counted, the target's row included.
// unit = q0 * C * S + u0 + blockIdx.x = ((target q) * C + direction chunk c) * S + slice sl;  acc[(q - q0) * k + r][le, ge]
template <int D>
__global__ __launch_bounds__(HS_THREADS) void hs_pairwise_kernel(const double *__restrict__ P, i64 n,
                                                                 const double *__restrict__ U, i64 k, PointSel sel, i64 q0,
                                                                 u64 u0, u64 C, u64 S, u32 *__restrict__ acc) {
    __shared__ double tile[HS_PTILE * D];
    const u64 u = u0 + blockIdx.x;
    const i64 ql = (i64)(u / (C * S));
    const i64 q = q0 + ql;
    const i64 c = (i64)(u / S % C);
    const i64 sl = (i64)(u % S);
    const PointView v = point_view(sel, P, n, D, q);
    const int *mem = v.mem;
    const double *xp = v.x;
    const i64 cnt = v.cnt;
    const i64 i_begin = sl * HS_SLICE;
    const i64 i_end = i_begin + HS_SLICE < cnt ? i_begin + HS_SLICE : cnt;
    if (i_begin >= i_end) return;                                  // (block-uniform) a shorter block of the members form
    const i64 r = c * HS_THREADS + threadIdx.x;
    const bool active = r < k;
    double x[D], uu[D];
#pragma unroll
    for (int e = 0; e < D; ++e) {
        x[e] = xp[e];
        uu[e] = active ? U[r * D + e] : 0.0;
    }
    const double zq = hs_proj<D>(x, uu);
    u32 le = 0, ge = 0;
    for (i64 i0 = i_begin; i0 < i_end; i0 += HS_PTILE) {
        const int tc = (int)(i_end - i0 < HS_PTILE ? i_end - i0 : HS_PTILE);
        __syncthreads();
        for (int y = threadIdx.x; y < tc * D; y += HS_THREADS) {
            const int pt = y / D, e = y % D;
            const i64 src = mem ? (i64)mem[i0 + pt] : i0 + pt;
            tile[y] = P[src * D + e];
        }
        __syncthreads();
        for (int j = 0; j < tc; ++j) {
            double y[D];
#pragma unroll
            for (int e = 0; e < D; ++e) y[e] = tile[j * D + e];    // every lane the same address: broadcast
            const double z = hs_proj<D>(y, uu);
            le += z <= zq ? 1u : 0u;
            ge += z >= zq ? 1u : 0u;
        }
    }
    if (active) {
        u32 *a = acc + ((u64)ql * (u64)k + (u64)r) * 2;
        atomicAdd(a, le);
        atomicAdd(a + 1, ge);
    }
}

// one workgroup per target of the batch: out[q0 + b] = min over directions of min(le, ge) (+ self)
__global__ __launch_bounds__(HS_THREADS) void hs_reduce_kernel(const u32 *__restrict__ acc, i64 k, u32 self,
                                                               i64 *__restrict__ out) {
    __shared__ u32 wmin[HS_THREADS / 64];
    const u32 *a = acc + (u64)blockIdx.x * (u64)k * 2;
    u32 v = 0xffffffffu;
    for (i64 r = threadIdx.x; r < k; r += HS_THREADS) {
        const u32 le = a[2 * r], ge = a[2 * r + 1];
        const u32 w = le < ge ? le : ge;
        v = w < v ? w : v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const u32 w = __shfl_down(v, o);
        v = w < v ? w : v;
    }
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < HS_THREADS / 64; ++j) v = wmin[j] < v ? wmin[j] : v;
        out[blockIdx.x] = (i64)v + (i64)self;
    }
}

template <int D>
static int launch_hs_pairwise_d(const double *P, i64 n, const double *U, i64 k, const PointSel &sel, i64 m, i64 *out, hipStream_t s) {
    const i64 cnt_max = sel_cnt_max(sel, n);
    const u64 C = (u64)((k + HS_THREADS - 1) / HS_THREADS);
    const u64 S = (u64)((cnt_max + HS_SLICE - 1) / HS_SLICE);
    i64 mq = (i64)(HS_ACC_BYTES / ((size_t)k * 8));                 // targets per batch: what the accumulator holds
    mq = mq < 1 ? 1 : mq > m ? m : mq;
    u32 *acc = nullptr;
    SD_HIP(hipMallocAsync((void **)&acc, (size_t)mq * k * 8, s));
    hipError_t err = hipSuccess;
    for (i64 q0 = 0; q0 < m && err == hipSuccess; q0 += mq) {
        const i64 mb = m - q0 < mq ? m - q0 : mq;
        err = hipMemsetAsync(acc, 0, (size_t)mb * k * 8, s);
        const u64 units = (u64)mb * C * S;
        for (u64 u0 = 0; u0 < units && err == hipSuccess; u0 += HS_UNITS) {
            const u64 g = units - u0 < HS_UNITS ? units - u0 : HS_UNITS;
            hipLaunchKernelGGL((hs_pairwise_kernel<D>), dim3((unsigned)g), dim3(HS_THREADS), 0, s, P, n, U, k, sel, q0, u0, C,
                               S, acc);
            err = hipGetLastError();
        }
        if (err != hipSuccess) break;
        hipLaunchKernelGGL(hs_reduce_kernel, dim3((unsigned)mb), dim3(HS_THREADS), 0, s, acc, k, sel.Q ? 1u : 0u, out + q0);
        err = hipGetLastError();
    }
    const hipError_t ferr = hipFreeAsync(acc, s);                  // freed on the error path too
    if (err != hipSuccess)
        return fail(SD_ERR_HIP, "halfspace launch failed: %s (%s:%d)", hipGetErrorString(err), __FILE__, __LINE__);
    SD_HIP(ferr);
    return SD_OK;
}

int launch_halfspace_counts(const double *P, i64 n, int d, const double *U, i64 k, const i64 *targets, i64 m, i64 *out,
                            void *ws, size_t ws_bytes, hipStream_t s) {
    if (d < 1 || d > 8) return fail(SD_ERR_UNSUPPORTED, "halfspace counts cover d in [1,8], got %d", d);
    return launch_hs_counts(P, n, d, U, k, targets, m, out, ws, ws_bytes, s);
}

int launch_halfspace_pairwise(const double *P, i64 n, int d, const double *U, i64 k, const PointSel &sel, i64 m, i64 *out,
                              hipStream_t s) {
    SD_DISPATCH_D(d, return launch_hs_pairwise_d<D_>(P, n, U, k, sel, m, out, s))
    return fail(SD_ERR_UNSUPPORTED, "halfspace counts cover d in [1,8], got %d", d);
}

}  // namespace sd
