// bd_strict_class.hip -- K3 strict band depth (relax=False, J = 2) of SHORT series by STATE CLASSES: O(n) per target, any n.
//
// strict_class_kernel (T <= 5, a histogram per lane) and strict_class_wg_kernel (3 <= T <= 8, NaN-free data, shared histograms) count
// the same classes; strict_any_nan_kernel tells which data is which.  Which form runs is the route plan's decision (strict_routes.h).
#include "sd_common.h"
#include "rank_routes.h"

namespace sd {

// ---------------------------------------------------------------------------------------------------
// J = 2 over at most three timepoints, any n: the L-infinity / box containment of point clouds (SURVEY 8 P4:
// FunctionalDepth([points.T]) -- "curves" = points, "timepoints" = coordinates; config 5 is 10^6 points in R^3, where
// the reference's default relax=False asks for the pairs of points whose bounding box contains the target).
// Per (target, other point) a STATE per coordinate in two bits -- above, below, neither (tie), both (NaN) -- i.e. a
// class c < 4^T; a pair is contained at every coordinate iff c_a & c_b == 0.  With h[c] = points per class,
//     ordered contained pairs = sum over c, c' with c & c' == 0 of h[c] h[c'] = sum over masks (-1)^popc(mask) U[mask]^2,
// U = superset sums of h (inclusion-exclusion over the 2T bits), so a target costs one pass over the points and a
// 64-entry transform -- O(n) per target instead of O(n^2), exact, no limit on n.
// Lanes = targets (coordinates in VGPRs, a private 4^T-counter histogram per lane in LDS: [class][lane], no atomics
// between lanes); the points stream through the scalar cache, eight per load, the same for every lane of the block.
// ---------------------------------------------------------------------------------------------------
constexpr int ST_CL_THREADS = 128;
// lanes (= targets) per block: the private histograms of a block must fit the LDS -- 3^T (NaN-free) or 4^T counters per lane
__host__ __device__ constexpr int st_cl_threads(int TT, bool NANS) {
    return TT <= 3 ? ST_CL_THREADS : (TT == 4 ? (NANS ? 64 : 128) : (NANS ? 32 : 64));
}

// is there a NaN anywhere in the data?  (flag[0] = 1)  NaN-free data -- the rule -- needs three states per coordinate
// instead of four: 27 counters per lane instead of 64 at T = 3, and 2.4 x the waves per SIMD that hide this kernel's
// LDS and scalar-load latencies.
__global__ __launch_bounds__(ST_THREADS) void strict_any_nan_kernel(const double *__restrict__ A, i64 na, const double *__restrict__ B,
                                                                   i64 nbv, u32 *__restrict__ flag) {
    bool isn = false;
    for (i64 i = (i64)blockIdx.x * ST_THREADS + threadIdx.x; i < na + nbv; i += (i64)gridDim.x * ST_THREADS) {
        const double v = i < na ? A[i] : B[i - na];
        isn |= v != v;
    }
    if (__syncthreads_or(isn) && threadIdx.x == 0) flag[0] = 1u;
}

template <int TT, bool NANS>
__global__ __launch_bounds__(st_cl_threads(TT, NANS)) void strict_class_kernel(const double *__restrict__ Y, i64 n, const i64 *__restrict__ targets,
                                                                    const double *__restrict__ Q, i64 m, const u32 *__restrict__ nanflag,
                                                                    u64 *__restrict__ out, int jcols) {
    if ((nanflag[0] != 0) != NANS) return;                                   // the other instantiation serves this data
    constexpr int P3 = TT == 1 ? 3 : (TT == 2 ? 9 : (TT == 3 ? 27 : (TT == 4 ? 81 : 243)));
    constexpr int NC = NANS ? (1 << (2 * TT)) : P3;
    constexpr int CLT = st_cl_threads(TT, NANS);
    __shared__ u32 hist[NC][CLT];
    const int tid = threadIdx.x;
    const i64 q = (i64)blockIdx.x * CLT + tid;
    const bool active = q < m;
    const i64 tg = (active && !Q) ? (targets ? targets[q] : q) : -1;        // its own column is not one of the others
    double x[TT];
    bool tnan = false;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
        x[t] = !active ? 0.0 : (Q ? Q[t * m + q] : Y[t * n + tg]);
        tnan |= x[t] != x[t];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) hist[c][tid] = 0;
    // Per (target, point): 2 T fp64 compares turned into the class code (two bits per coordinate, NaN coordinates of the
    // point -- a scalar: the point is the same for every lane -- set both; or base 3 without NaN), one increment of the
    // lane's own counter.  The target meets itself in the stream (class 0: every coordinate ties) and is taken off
    // afterwards.  (Measured and not kept: compare + add-with-carry chains, one instruction per bit instead of two, and
    // ds_add instead of read / add / write: 1.9 and 1.8 s against 1.46 s at 10^6 points.)
    auto visit = [&](const double (&p)[TT]) {
        u32 code = 0;
        if constexpr (NANS) {
            u32 nanbits = 0;
#pragma unroll
            for (int t = TT - 1; t >= 0; --t) {
                const unsigned long long pb = (unsigned long long)__double_as_longlong(p[t]);
                const u32 hi = (u32)(pb >> 32) & 0x7FFFFFFFu, lo = (u32)pb;     // 32-bit tests: scalar ALU
                nanbits = (nanbits << 2) | ((hi > 0x7FF00000u || (hi == 0x7FF00000u && lo != 0u)) ? 3u : 0u);
                code |= (p[t] > x[t] ? 1u : 0u) << (2 * t);                      // above
                code |= (p[t] < x[t] ? 2u : 0u) << (2 * t);                      // below
            }
            code |= nanbits;
        } else {
#pragma unroll
            for (int t = TT - 1; t >= 0; --t) code = code * 3u + (p[t] > x[t] ? 1u : 0u) + (p[t] < x[t] ? 2u : 0u);
        }
        hist[code][tid] += 1u;                                               // own counter: no atomic needed
    };
    i64 i = 0;
    for (; i + 8 <= n; i += 8) {
        double blkp[TT][8];
#pragma unroll
        for (int t = 0; t < TT; ++t)
#pragma unroll
            for (int k = 0; k < 8; ++k) blkp[t][k] = Y[t * n + i + k];      // wave-uniform addresses: scalar loads
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double p[TT];
#pragma unroll
            for (int t = 0; t < TT; ++t) p[t] = blkp[t][k];
            visit(p);
        }
    }
    for (; i < n; ++i) {
        double p[TT];
#pragma unroll
        for (int t = 0; t < TT; ++t) p[t] = Y[t * n + i];
        visit(p);
    }
    if (!active) return;
    if (tg >= 0 && !tnan) hist[0][tid] -= 1u;                                // the target itself (a NaN target counts nothing)
    // class 0 = the points that tie with the target in every coordinate: the only ones compatible with themselves
    const u64 ties = hist[0][tid];
    long long total = 0;
    if constexpr (NANS) {
        // superset sums over the 2T bits, in place, then inclusion-exclusion
#pragma unroll
        for (int bit = 1; bit < NC; bit <<= 1)
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (!(c & bit)) hist[c][tid] += hist[c | bit][tid];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const long long u = (long long)hist[c][tid];
            total += (__builtin_popcount((unsigned)c) & 1) ? -u * u : u * u;
        }
    } else if constexpr (TT >= 4) {
        // three states, 81 / 243 classes: too many for registers.  A pair is compatible iff in no coordinate both are above or
        // both below: prod_t (1 - [both above at t] - [both below at t]) = sum over subsets S of the coordinates of (-1)^|S| [equal
        // and strict on S].  In place, per coordinate, the tie slot becomes the sum of the three states (a wild card); entry c
        // then counts the points that match c's strict digits, and the ordered pairs are sum_c (-1)^(strict digits of c) entry(c)^2.
#pragma unroll 1
        for (int stride = 1; stride < NC; stride *= 3)
#pragma unroll 1
            for (int g = 0; g < NC / 3; ++g) {
                const int base = (g / stride) * stride * 3 + (g % stride);
                hist[base][tid] += hist[base + stride][tid] + hist[base + 2 * stride][tid];
            }
#pragma unroll 1
        for (int c = 0; c < NC; ++c) {
            int strict_digits = 0;
            for (int d = c; d; d /= 3) strict_digits += (d % 3) != 0;
            const long long u = (long long)hist[c][tid];
            total += (strict_digits & 1) ? -u * u : u * u;
        }
    } else {
        // three states: z = (M x ... x M) h in registers (tie ~ all, above ~ {tie, below}, below ~ {tie, above}), then h . z
        u64 h[NC], z[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) { h[c] = hist[c][tid]; z[c] = h[c]; }
#pragma unroll
        for (int stride = 1; stride < NC; stride *= 3)
#pragma unroll
            for (int g = 0; g < NC / 3; ++g) {
                const int base = (g / stride) * stride * 3 + (g % stride);
                const u64 s0 = z[base], s1 = z[base + stride], s2 = z[base + 2 * stride];
                z[base] = s0 + s1 + s2;
                z[base + stride] = s0 + s2;
                z[base + 2 * stride] = s0 + s1;
            }
#pragma unroll
        for (int c = 0; c < NC; ++c) total += (long long)(h[c] * z[c]);
    }
    out[q * jcols] = tnan ? 0ull : ((u64)total - ties) / 2;                  // NaN in the target: nothing is contained
}

// ---------------------------------------------------------------------------------------------------
// J = 2 over 6 ... 8 timepoints, NaN-free data, any n: the same state classes, counted by a WORKGROUP per G targets.
// Lanes = points (their coordinates in VGPRs, SCW_PTS points per thread and trip, coalesced loads that serve all G targets);
// the target's coordinates are wave-uniform (SGPRs), a pair costs 2 T compares, the base-3 code and one LDS atomic on the
// target's histogram (3^T counters).  Then the in-place wild-card transform of strict_class_kernel, coordinate by
// coordinate with the workgroup's threads, and sum_c (-1)^(strict digits of c) entry(c)^2.
// ---------------------------------------------------------------------------------------------------
constexpr int SCW_PTS = 4;
template <int TT> struct ScwCfg {
    static constexpr int NC = TT == 3 ? 27 : (TT == 4 ? 81 : (TT == 5 ? 243 : (TT == 6 ? 729 : (TT == 7 ? 2187 : 6561))));
    static constexpr int G = TT <= 5 ? 16 : (TT <= 7 ? 8 : 4);          // (T >= 6:) 46 / 70 / 105 KB of histograms
    static constexpr int NT = TT == 8 ? 1024 : 512;                     // three / two / one workgroup per CU
    // few classes: the lanes of a wave meet on the same counter (most points are strictly above or below in every coordinate:
    // 2^T classes) and the LDS serialises them -- R copies of a target's histogram, a lane counts into copy lane % R
    // T = 6: 8 targets x 2 copies against 16 x 1: 10.1 against 15.6 ms on random walks (correlated coordinates: fewer classes
    // occur), the same on independent ones; T = 7 / 8 with copies (4 x 2 / 2 x 2 targets): 13.2 / 23.3 against 15.1 / 20.0 on walks,
    // 13.1 / 23.4 against 12.2 / 18.5 on independent coordinates -- not taken
    // (T = 3: 16 copies; 8 the same, 32 slower; 32 targets per workgroup slower)
    static constexpr int R = TT == 3 ? 16 : (TT == 4 ? 8 : (TT == 5 ? 4 : (TT == 6 ? 2 : 1)));
    static constexpr size_t LDS = (size_t)G * R * NC * 4;
};
__device__ __forceinline__ double scw_uniform(double v) {               // a wave-uniform double into SGPRs
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)(u32)b), hi = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

template <int TT>
__global__ __launch_bounds__(ScwCfg<TT>::NT) void strict_class_wg_kernel(const double *__restrict__ Y, i64 n,
                                                                         const i64 *__restrict__ targets,
                                                                         const double *__restrict__ Q, i64 m,
                                                                         const u32 *__restrict__ nanflag,
                                                                         u64 *__restrict__ out, int jcols) {
    if (nanflag && nanflag[0] != 0) return;                             // (T <= 5: the four-state kernel serves this data)
    using C = ScwCfg<TT>;
    constexpr int NC = C::NC, G = C::G, NT = C::NT, NW = NT / 64, R = C::R, GS = R * NC;
    extern __shared__ u32 scw_hist[];                                   // [G][R][NC]
    __shared__ double xs[G][8];
    __shared__ long long red[G][NW];
    __shared__ u32 s_ties[G];
    u32 *hist = scw_hist;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const i64 q0 = (i64)blockIdx.x * G;
    const int gc = (int)(m - q0 < G ? m - q0 : G);                      // targets of this workgroup
    for (int c = tid; c < G * GS; c += NT) hist[c] = 0;
    if (tid < G * TT) {
        const int g = tid / TT, t = tid % TT;
        double v = 0.0;
        if (g < gc) {
            const i64 q = q0 + g;
            v = Q ? Q[t * m + q] : Y[t * n + (targets ? targets[q] : q)];
        }
        xs[g][t] = v;
    }
    __syncthreads();
    for (i64 i0 = tid; i0 < n; i0 += (i64)NT * SCW_PTS) {
        double p[SCW_PTS][TT];
        bool ok[SCW_PTS];
#pragma unroll
        for (int k = 0; k < SCW_PTS; ++k) {
            const i64 i = i0 + (i64)k * NT;
            ok[k] = i < n;
#pragma unroll
            for (int t = 0; t < TT; ++t) p[k][t] = ok[k] ? Y[t * n + i] : 0.0;
        }
#pragma unroll 1
        for (int g = 0; g < gc; ++g) {
            double x[TT];
#pragma unroll
            for (int t = 0; t < TT; ++t) x[t] = scw_uniform(xs[g][t]);
            u32 *hg = hist + g * GS + (lane & (R - 1)) * NC;
#pragma unroll
            for (int k = 0; k < SCW_PTS; ++k) {
                u32 code = 0;
#pragma unroll
                for (int t = TT - 1; t >= 0; --t) code = code * 3u + (p[k][t] > x[t] ? 1u : 0u) + (p[k][t] < x[t] ? 2u : 0u);
                if (ok[k]) atomicAdd(&hg[code], 1u);
            }
        }
    }
    __syncthreads();
    // the target itself met in the stream as class 0 (every coordinate ties): taken off; class 0 = the points that tie with
    // the target everywhere, the only ones compatible with themselves
    if constexpr (R > 1) {
        for (int w = tid; w < gc * NC; w += NT) {
            u32 *h = hist + (w / NC) * GS + (w % NC);
            u32 v = h[0];
#pragma unroll
            for (int r = 1; r < R; ++r) v += h[r * NC];
            h[0] = v;
        }
        __syncthreads();
    }
    if (tid < gc) {
        const bool self = !Q && (targets ? targets[q0 + tid] : q0 + tid) >= 0;
        if (self) hist[tid * GS] -= 1u;
        s_ties[tid] = hist[tid * GS];
    }
    __syncthreads();
    // per coordinate the tie slot becomes the sum of the three states (see strict_class_kernel)
#pragma unroll 1
    for (int stride = 1; stride < NC; stride *= 3) {
        for (int w = tid; w < gc * (NC / 3); w += NT) {
            const int g = w / (NC / 3), idx = w % (NC / 3);
            u32 *h = hist + g * GS + (idx / stride) * stride * 3 + (idx % stride);
            h[0] += h[stride] + h[2 * stride];
        }
        __syncthreads();
    }
    long long acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = 0;
    for (int c = tid; c < NC; c += NT) {
        int strict_digits = 0;
#pragma unroll
        for (int t = 0, d = c; t < TT; ++t, d /= 3) strict_digits += (d % 3) != 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const long long u = (long long)hist[g * GS + c];
            acc[g] += (strict_digits & 1) ? -u * u : u * u;
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        long long v = acc[g];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        if (lane == 0) red[g][wave] = v;
    }
    __syncthreads();
    if (tid < gc) {
        long long total = 0;
        for (int w = 0; w < NW; ++w) total += red[tid][w];
        out[(q0 + tid) * jcols] = ((u64)total - (u64)s_ties[tid]) / 2;
    }
}

template <int TT>
static int launch_class_wg(const double *Y, i64 n, const i64 *targets, const double *Q, i64 m, const u32 *nanflag, u64 *out, int jcols,
                           hipStream_t s) {
    using C = ScwCfg<TT>;
    auto k = strict_class_wg_kernel<TT>;
    SD_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS));
    hipLaunchKernelGGL(k, dim3((unsigned)((m + C::G - 1) / C::G)), dim3(C::NT), C::LDS, s, Y, n, targets, Q, m, nanflag, out, jcols);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

void launch_strict_any_nan(const double *Y, i64 T, i64 n, const double *Q, i64 m, u32 *flag, hipStream_t s) {
    hipLaunchKernelGGL(strict_any_nan_kernel, dim3(1024), dim3(ST_THREADS), 0, s, Y, T * n, Q ? Q : Y, Q ? T * m : (i64)0, flag);
}

int launch_bd_strict_class_wg(const double *Y, i64 T, i64 n, const i64 *targets, const double *Q, i64 m, const u32 *nanflag,
                              u64 *out, int jcols, hipStream_t s) {
    switch ((int)T) {
        case 3: return launch_class_wg<3>(Y, n, targets, Q, m, nanflag, out, jcols, s);
        case 4: return launch_class_wg<4>(Y, n, targets, Q, m, nanflag, out, jcols, s);
        case 5: return launch_class_wg<5>(Y, n, targets, Q, m, nanflag, out, jcols, s);
        case 6: return launch_class_wg<6>(Y, n, targets, Q, m, nanflag, out, jcols, s);
        case 7: return launch_class_wg<7>(Y, n, targets, Q, m, nanflag, out, jcols, s);
        case 8: return launch_class_wg<8>(Y, n, targets, Q, m, nanflag, out, jcols, s);
        default: return fail(SD_ERR_UNSUPPORTED, "the workgroup form of the class kernel covers three to eight timepoints");
    }
}

// strict_class_kernel<TT, NANS> with its own grid and block
template <int TT, bool NANS>
static void launch_class_lanes(const double *Y, i64 n, const i64 *targets, const double *Q, i64 m, const u32 *flag, u64 *out,
                               int jcols, hipStream_t s) {
    constexpr int NT = st_cl_threads(TT, NANS);
    hipLaunchKernelGGL((strict_class_kernel<TT, NANS>), dim3((unsigned)((m + NT - 1) / NT)), dim3(NT), 0, s, Y, n, targets, Q, m, flag,
                       out, jcols);
}
// the lane kernel of T <= 5 timepoints, three-state (NANS = false: returns at once when the flag is set) or four-state (when not)
template <bool NANS>
static void launch_class_lanes_of(i64 T, const double *Y, i64 n, const i64 *targets, const double *Q, i64 m, const u32 *flag,
                                  u64 *out, int jcols, hipStream_t s) {
    switch ((int)T) {
        case 1: return launch_class_lanes<1, NANS>(Y, n, targets, Q, m, flag, out, jcols, s);
        case 2: return launch_class_lanes<2, NANS>(Y, n, targets, Q, m, flag, out, jcols, s);
        case 3: return launch_class_lanes<3, NANS>(Y, n, targets, Q, m, flag, out, jcols, s);
        case 4: return launch_class_lanes<4, NANS>(Y, n, targets, Q, m, flag, out, jcols, s);
        default: return launch_class_lanes<5, NANS>(Y, n, targets, Q, m, flag, out, jcols, s);
    }
}

int launch_bd_strict_classes(const StrictPlan &plan, const double *Y, i64 T, i64 n, const i64 *targets, const double *Q, i64 m,
                             u64 *out, int jcols, void *ws, size_t ws_bytes, hipStream_t s) {
    if (T < 1 || T > 5) return fail(SD_ERR_UNSUPPORTED, "the class kernel covers up to five timepoints");
    Carver cv(ws, ws_bytes);
    u32 *flag = (u32 *)cv.take(256);
    if (!flag) return fail(SD_ERR_WORKSPACE, "strict-depth workspace too small");
    SD_HIP(hipMemsetAsync(flag, 0, 4, s));
    if (plan.grid && ws_bytes >= bd_strict_grid_workspace_bytes(T, n, targets != nullptr)) {
        // two to four coordinates at large n: the grid of cells (bd_strict_grid.hip) when the workspace holds it (a caller that
        // passed the floor keeps the O(m n) kernels); it sets the flag itself from the rank route's NaN counts
        if (int rc = launch_bd_strict_grid(Y, T, n, targets, m, out, jcols, flag, ws, ws_bytes, s)) return rc;
    } else {
        launch_strict_any_nan(Y, T, n, Q, m, flag, s);
        // NaN-free data, T = 3, 4, 5: the workgroup form (lanes = points, shared histograms: 10^5 x 3 / 4 / 5 in 4.9 / 6.7 / 8.5 ms
        // against 10.7 / 21 / 46 with a histogram per lane; 10^6 x 3: 427 against 506 ms); T = 1, 2 -- or all of them when the
        // plan says so (cross-check builds) -- the three-state lane kernel
        if (T <= 2 || plan.laneclass) launch_class_lanes_of<false>(T, Y, n, targets, Q, m, flag, out, jcols, s);
        else if (int rc = launch_bd_strict_class_wg(Y, T, n, targets, Q, m, flag, out, jcols, s)) return rc;
    }
    // data with NaN (the flag is set): the four-state lane kernel, which returns at once otherwise
    launch_class_lanes_of<true>(T, Y, n, targets, Q, m, flag, out, jcols, s);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

}  // namespace sd
