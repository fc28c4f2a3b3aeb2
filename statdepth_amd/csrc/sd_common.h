// sd_common.h -- shared declarations of the gfx950 band-depth engine (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "statdepth_hip.h"

typedef unsigned long long u64;
typedef int64_t i64;
typedef unsigned int u32;

namespace sd {

constexpr int JMAX_HOST = 8;   // J range of the count kernels

// thread-local error message returned by sd_last_error()
void set_error(const char *fmt, ...);
int fail(int code, const char *fmt, ...);

#define SD_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return sd::fail(SD_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                            __FILE__, __LINE__);                                              \
    } while (0)

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// carve-out helper for the caller-provided workspace
struct Carver {
    char *base;
    size_t off, cap;
    Carver(void *p, size_t bytes) : base((char *)p), off(0), cap(bytes) {}
    void *take(size_t bytes) {
        size_t o = align_up(off, 256);
        if (!base || o + bytes > cap) { off = cap + 1; return nullptr; }
        off = o + bytes;
        return base + o;
    }
    size_t rest() const { size_t o = align_up(off, 256); return o < cap ? cap - o : 0; }   // what the next take() could get
    bool ok() const { return off <= cap; }
};

// Value of an environment switch that selects an alternative implementation for cross-checks (SD_RANK_IMPL,
// SD_BIG_IMPL, SD_SIMPLEX_GENERIC, ...).  The product library (libstatdepth_hip.so) is built without -DSD_CROSSCHECK:
// there this returns 0 for every name and no environment variable is read; libstatdepth_hip_xcheck.so (tests only)
// reads the variable on every call.  xcheck.hip.
long long xswitch(const char *name);

// compute units of the current device (256 when the runtime does not say), and how many of them the stream may use (its
// CU mask, when it has one that names fewer).  sd_api.hip.
int device_cus();
int stream_cus(hipStream_t s);

// ---- launchers implemented in the kernel translation units ----
// strided (t,i) -> time-major Y[t*n+i]
int launch_to_time_major(const double *X, i64 T, i64 n, i64 st, i64 sn, double *Y, hipStream_t s);
// per-row NaN counts of a time-major matrix, plus a global any-NaN counter
int launch_nan_count_rows(const double *Y, i64 T, i64 n, u32 *nan_cnt, hipStream_t s);
// K1+K2 pairwise
// targets == nullptr means the contiguous block [tbegin, tbegin + m)
int launch_mbd_pairwise(const double *Y, i64 T, i64 n, const i64 *targets, i64 tbegin, i64 m, int J,
                        const u32 *nan_cnt, u64 *out, hipStream_t s);
// external targets Q (T x m, time-major) against the n curves of Y
int launch_mbd_external(const double *Y, i64 T, i64 n, const double *Q, i64 m, int J, const u32 *nan_cnt, u64 *out,
                        hipStream_t s);
int launch_mbd_subsets(const double *Y, i64 T, i64 n, const int *members, i64 nb, int bs, const int *target, int J,
                       u64 *out, hipStream_t s);
int launch_above_below(const double *Y, i64 T, i64 n, const i64 *targets, i64 m, u32 *AB, hipStream_t s);
bool bd_strict_subsets_supported(i64 T, int bs);
size_t bd_strict_subsets_workspace_bytes(i64 T, i64 nb, int bs);
int launch_bd_strict_subsets(const double *Y, i64 T, i64 n, const int *members, i64 nb, int bs, const int *target, u64 *out,
                             void *ws, size_t ws_bytes, hipStream_t s);
// K1+K2 rank formulation: the route plan and its launcher are in rank_routes.h
// external targets through the bucket structure (n <= 16384, J <= 3)
bool mbd_rank_external_supported(i64 T, i64 n, i64 m, int J);
size_t mbd_rank_external_workspace_bytes(i64 T, i64 n, i64 m, int J);
int launch_mbd_external_rank(const double *Y, i64 T, i64 n, const double *Q, i64 m, int J, u64 *out, void *ws,
                             size_t ws_bytes, hipStream_t s);
// K1+K2 rank formulation for n > 16384 (chunked): what the strict path and the route plan size its scratch by
bool mbd_rank_big_supported(i64 T, i64 n, int J);
size_t mbd_rank_big_workspace_bytes(i64 T, i64 n, int J);
// K3 strict
size_t bd_strict_workspace_bytes(i64 T, i64 n, i64 m, int J);
size_t bd_strict_min_workspace_bytes(i64 T, i64 n, i64 m, int J);
size_t bd_strict_nanfree_workspace_bytes(i64 T, i64 n, i64 m, int J);
size_t bd_strict_launch_floor_bytes(i64 T, i64 n, i64 m, int J);    // what launch_bd_strict needs at least to be called
int launch_bd_strict(const double *Y, i64 T, i64 n, const i64 *targets, i64 m, int J,
                     u64 *out, void *ws, size_t ws_bytes, hipStream_t s);
size_t bd_strict_external_workspace_bytes(i64 T, i64 n, i64 m);
int launch_bd_strict_external(const double *Y, i64 T, i64 n, const double *Q, i64 m, u64 *out, void *ws, size_t ws_bytes,
                              hipStream_t s);
// The point-cloud launchers below take the selection of the m targets (rows of P, external points, or blocks of rows)
// as a PointSel: point_select.h.
struct PointSel;
// K5 l1
int launch_l1(const double *P, i64 n, int d, const PointSel &sel, i64 m, double *out, hipStream_t s);
// K4 simplex (samples < 0: every subset; the sampled estimator takes the rows form only)
int launch_pointcloud_simplex(const double *P, i64 n, int d, const PointSel &sel, i64 m, double tol,
                              i64 samples, u64 seed, u64 *out, hipStream_t s, void *ws = nullptr, size_t ws_bytes = 0);
int launch_multi_simplex(const double *P, i64 n, i64 T, int d, const i64 *targets, i64 m, int relax,
                         double tol, i64 samples, u64 seed, u64 *out, hipStream_t s, void *ws = nullptr, size_t ws_bytes = 0);
// records of the sampled estimators' shared factorisation (a batch of (timepoint, sample) pairs)
size_t simplex_sampled_workspace_bytes(i64 n, i64 T, int d, i64 samples);
// SD_SIMPLEX_GENERIC = 1: one launch of the per-target route, targets [q0, q0 + grid.y), on the retired generic kernel.  A
// hook like those of rank_routes.h: defined next to the kernel in simplex_retired.hip (cross-check library only); in the
// product xcheck.hip defines it to fail with SD_ERR_UNSUPPORTED, and nothing calls it there.
int retired_simplex_generic(const double *P, i64 n, i64 T, int d, const PointSel &sel, int relax, double tol, u64 total,
                            u64 per_thread, i64 samples, u64 seed, i64 q0, u64 *out, dim3 grid, hipStream_t s);

// K6 componentwise band containment of multivariate curves (band_enum.hip)
bool multi_band_supported(i64 n, i64 T, int d);
size_t multi_band_workspace_bytes(i64 n, i64 T, int d);
int launch_multi_band(const double *P, i64 n, i64 T, int d, const i64 *targets, i64 m, u64 *out, void *ws, size_t ws_bytes,
                      hipStream_t s);
// every j = 2 .. J in one pass (J in [2, 4], checked by the caller): out[q * (J - 1) + j - 2]
int launch_multi_band_j(const double *P, i64 n, i64 T, int d, const i64 *targets, i64 m, int J, u64 *out, void *ws,
                        size_t ws_bytes, hipStream_t s);

// K7 Oja volume sums (oja.hip): out = sum of |det| / d! over the d-subsets of the others
int launch_oja(const double *P, i64 n, int d, const PointSel &sel, i64 m, double *out, hipStream_t s);

// K8 probabilistic depths (prob_depth.hip): unnormalised sums of the reference's normal and Poisson depths
int launch_prob_normal_sums(const double *mu, const double *sigma, i64 n, const i64 *targets, i64 m, double *out,
                            hipStream_t s);
int launch_prob_poisson_sums(const double *lam, i64 T, i64 n, i64 lim, const i64 *targets, i64 m, double *out, hipStream_t s);
// adds part[0 .. u1 - u0) of units [u0, u1) (unit u = target u / S, chunk u % S) into out[u / S] in unit order; out holds
// the running sum of a target whose chunks span launches
hipError_t launch_prob_fold(const double *part, u64 u0, u64 u1, u64 S, double *out, hipStream_t s);
// K9 band depth of curves under Gaussian noise (prob_band.hip): unnormalised pair sums (sd_prob_band_sums)
int launch_prob_band_sums(const double *mu, const double *var, i64 T, i64 n, const i64 *targets, i64 m, const int *members,
                          int bs, int relax, double *out, hipStream_t s);

// K10 halfspace (Tukey) depth over a fixed direction set (halfspace.hip): out = min over directions of min(le, ge)
size_t halfspace_workspace_bytes(i64 n, i64 k);
size_t halfspace_min_workspace_bytes(i64 n);
int launch_halfspace_counts(const double *P, i64 n, int d, const double *U, i64 k, const i64 *targets, i64 m, i64 *out,
                            void *ws, size_t ws_bytes, hipStream_t s);
int launch_halfspace_pairwise(const double *P, i64 n, int d, const double *U, i64 k, const PointSel &sel, i64 m, i64 *out,
                              hipStream_t s);

// K11 exact halfspace depth in the plane (halfspace_exact.hip): route 1 = angular sweep in LDS, 2 = pairwise L/R/S/O
constexpr i64 HX_SWEEP_CAPACITY = 8192;                             // sample points one sweep workgroup holds
int halfspace2_route(int algo, i64 cnt_max);                       // 0: algo = 1 (sweep) above the capacity
double halfspace2_work(int route, i64 m, i64 cnt_max);             // predicate evaluations
int launch_halfspace2(const double *P, i64 n, const PointSel &sel, i64 m, int route, i64 *out, hipStream_t s);

// K13 exact simplicial depth in the plane (simplicial_exact.hip): route 1 = angular sweep in LDS, 2 = pairwise e_j
constexpr i64 SX_SWEEP_CAPACITY = 8192;                             // others one sweep workgroup holds
int simplicial2_route(int algo, i64 others_max);                   // 0: algo = 1 (sweep) above the capacity
double simplicial2_work(int route, i64 m, i64 others_max);         // predicate evaluations
i64 simplicial2_max_others();                                      // the most others whose C(others, 3) fits int64
int launch_simplicial2(const double *P, i64 n, const PointSel &sel, i64 m, int route, i64 *out, hipStream_t s);

// K12 projection depth (projection.hip): out = max over directions of |z - med| / mad.  launch_projection_sorted serves
// the rows and the external form (sel), launch_projection_blocks the blocks form (sel.bs <= PD_MAX_BLOCK: the caller checks)
constexpr int PD_MAX_BLOCK = 2048;                                  // members of a block: what pd_blocks_kernel sorts in LDS
size_t projection_workspace_bytes(i64 n, i64 k);
size_t projection_min_workspace_bytes(i64 n);
int launch_projection_sorted(const double *P, i64 n, int d, const double *U, i64 k, const PointSel &sel, i64 m, double *out,
                             void *ws, size_t ws_bytes, hipStream_t s);
int launch_projection_blocks(const double *P, i64 n, int d, const double *U, i64 k, const PointSel &sel, i64 nb, double *out,
                             hipStream_t s);

// K14 rank depths, K15 extremal depth and K17 total variation depth of curves: the pair-image plan and the launchers are in
// curve_routes.h; so are the plan and the launchers of K20 (squared L2 distances of curves, curve_dist.hip)

// K16 central regions, fence, outside counts and whiskers of the functional boxplot (central_regions.hip).  Y time-major;
// fence, outside and whisker may be null (all three are with box = -1).  The workspace behind the time-major copy: a
// fence (16 T bytes), the counts (8 n) and, above the row capacity, the column blocks' min / max (16 T L per block)
constexpr i64 CR_ROW_CAPACITY = 16384;                              // curves of one row a workgroup holds in registers
size_t central_regions_workspace_bytes(i64 T, i64 n, int L);
int launch_central_regions(const double *Y, i64 T, i64 n, const uint8_t *level, int L, int box, double factor, double *env,
                           double *fence, int32_t *outside, double *whisker, void *ws, size_t ws_bytes, hipStream_t s);

// K18 halfspace and projection depth of multivariate curves over time (multi_cloud.hip): out = m x 2 records, (SH, MH)
// int64 or (PS, OM) double.  route 1 = a cloud's projections ranked in one workgroup's LDS, 2 = K10's / K12's launchers
// per timepoint
constexpr i64 MC_LDS_CAPACITY = 8192;                               // curves whose projections one workgroup sorts in LDS
int multi_cloud_route(int algo, i64 n);                            // 0: algo = 1 (lds) above the capacity
// extra: bytes per timepoint of a batch that the batch consumer asks for itself (McBatch::extra), padded to 256 as a whole
size_t multi_cloud_workspace_bytes(int route, bool proj, i64 n, i64 T, int d, i64 k, size_t extra = 0);
size_t multi_cloud_min_workspace_bytes(int route, bool proj, i64 n, int d, size_t extra = 0);
int launch_multi_cloud(bool proj, int route, const double *P, i64 n, i64 T, int d, const double *U, i64 k, const i64 *targets,
                       i64 m, void *out, void *ws, size_t ws_bytes, hipStream_t s);
// (the batch loop that both families and K19 share: multi_cloud_batches.h)

// K19 directional outlyingness of multivariate curves (directional_out.hip), a consumer of K18's projection batches: out =
// m x (d + 1) Welford records (M_0 .. M_(d-1), Q); centres (T) and curves (m x T x d) may be null
constexpr size_t DO_EXTRA = 8;                                     // Cn[tb]: the centre of each timepoint of the batch, int64
int launch_multi_outlyingness(int route, const double *P, i64 n, i64 T, int d, const double *U, i64 k, const i64 *targets, i64 m,
                              double *out, i64 *centres, double *curves, void *ws, size_t ws_bytes, hipStream_t s);

// exact C(a,k) on the host in u64 with overflow detection (returns false on overflow)
bool binom_u64_checked(u64 a, int k, u64 *out);

}  // namespace sd

// ---- device helpers -------------------------------------------------------
#ifdef __HIPCC__
namespace sd {

constexpr int JMAX = 8;

// C(a,k) for k = 0..K by the exact recurrence C(a,k) = C(a,k-1)*(a-k+1)/k.
// Caller guarantees k*C(a,k) < 2^64 (checked on the host from n, J, T).
template <int K>
__device__ __forceinline__ void binoms(u64 a, u64 (&c)[K + 1]) {
    c[0] = 1;
#pragma unroll
    for (int k = 1; k <= K; ++k) c[k] = c[k - 1] * (a - (u64)(k - 1)) / (u64)k;
}

// number of j-subsets (j = 2..J) of the n-1 other curves whose band contains the
// target at one timepoint, from A (above), B (below), N (NaN others), nm1 = n-1.
// acc[j-2] += count.  Restates oracle_mbd_counts (oracle/oracle.c).
template <int J>
__device__ __forceinline__ void band_counts_add(u32 A, u32 B, u32 N, u64 nm1, u64 (&acc)[JMAX - 1]) {
    u64 v = nm1 - N;
    if (N == 0) {
        if constexpr (J == 2) {
            acc[0] += (v * (v - 1) >> 1) - ((u64)A * (A - 1) >> 1) - ((u64)B * (B - 1) >> 1);
        } else {
            u64 cv[J + 1], ca[J + 1], cb[J + 1];
            binoms<J>(v, cv);
            binoms<J>(A, ca);
            binoms<J>(B, cb);
#pragma unroll
            for (int j = 2; j <= J; ++j) acc[j - 2] += cv[j] - ca[j] - cb[j];
        }
    } else {
        u64 cv[J + 1], ca[J + 1], cb[J + 1], cn[J + 1];
        binoms<J>(v, cv);
        binoms<J>(A, ca);
        binoms<J>(B, cb);
        binoms<J>(N, cn);
#pragma unroll
        for (int j = 2; j <= J; ++j) {
            u64 s = 0;
#pragma unroll
            for (int k = 1; k <= j; ++k) s += cn[j - k] * (cv[k] - ca[k] - cb[k]);
            acc[j - 2] += s;
        }
    }
}

// dispatch a runtime J in [2, JMAX] to a template instantiation
#define SD_DISPATCH_J(J, ...)                         \
    switch (J) {                                      \
        case 2: { constexpr int J_ = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int J_ = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int J_ = 4; __VA_ARGS__; } break; \
        case 5: { constexpr int J_ = 5; __VA_ARGS__; } break; \
        case 6: { constexpr int J_ = 6; __VA_ARGS__; } break; \
        case 7: { constexpr int J_ = 7; __VA_ARGS__; } break; \
        case 8: { constexpr int J_ = 8; __VA_ARGS__; } break; \
        default: return sd::fail(SD_ERR_INVALID, "J=%d outside [2,8]", (int)(J)); \
    }

// dispatch a runtime d in [1, 8] to a template instantiation; any other d falls through (the caller says what it covers)
#define SD_DISPATCH_D(d, ...)                         \
    switch (d) {                                      \
        case 1: { constexpr int D_ = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int D_ = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int D_ = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int D_ = 4; __VA_ARGS__; } break; \
        case 5: { constexpr int D_ = 5; __VA_ARGS__; } break; \
        case 6: { constexpr int D_ = 6; __VA_ARGS__; } break; \
        case 7: { constexpr int D_ = 7; __VA_ARGS__; } break; \
        case 8: { constexpr int D_ = 8; __VA_ARGS__; } break; \
    }

}  // namespace sd
#endif
