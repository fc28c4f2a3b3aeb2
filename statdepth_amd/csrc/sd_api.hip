// sd_api.hip -- the extern "C" boundary declared in include/statdepth_hip.h.
// Argument validation, workspace carving and kernel sequencing; no arithmetic.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "sd_common.h"
#include "statdepth_hip_projections.h"
#include "rank_routes.h"
#include "curve_routes.h"
#include "point_select.h"

namespace sd {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int device_cus() {
    static int cached[64];                                // per device; 0 = not asked yet (benign race: same value)
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        if (dev >= 0 && dev < 64 && cached[dev] > 0) return cached[dev];
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
        if (dev >= 0 && dev < 64) cached[dev] = cus;
    }
    return cus;
}

int stream_cus(hipStream_t s) {
    int usable = device_cus();
    uint32_t mask[16] = {0};
    if (hipExtStreamGetCUMask(s, 16, mask) == hipSuccess) {
        int bits = 0;
        for (int i = 0; i < 16; ++i) bits += __builtin_popcount(mask[i]);
        if (bits > 0 && bits < usable) usable = bits;
    } else {
        (void)hipGetLastError();
    }
    return usable;
}

bool binom_u64_checked(u64 a, int k, u64 *out) {
    if (k < 0 || (u64)k > a) { *out = 0; return true; }
    unsigned __int128 c = 1;
    for (int j = 1; j <= k; ++j) {
        c = c * (a - (u64)j + 1) / (u64)j;
        if (c >> 64) return false;
    }
    *out = (u64)c;
    return true;
}

// J, n, T limits shared by the count kernels: totals must fit int64 and the
// device recurrence C(a,k) = C(a,k-1)*(a-k+1)/k must not overflow u64.
static int check_count_range(i64 T, i64 n, int J) {
    if (J < 2 || J > JMAX_HOST) return fail(SD_ERR_INVALID, "J=%d outside [2,%d]", J, JMAX_HOST);
    u64 c;
    if (!binom_u64_checked((u64)(n > 0 ? n - 1 : 0), J, &c))
        return fail(SD_ERR_OVERFLOW, "C(n-1,J) overflows 64 bits (n=%lld, J=%d)", (long long)n, J);
    unsigned __int128 tot = (unsigned __int128)c * (u64)(T > J ? T : J);
    if (tot >> 63)
        return fail(SD_ERR_OVERFLOW, "T*C(n-1,J) >= 2^63 (T=%lld, n=%lld, J=%d): int64 totals would overflow",
                    (long long)T, (long long)n, J);
    return SD_OK;
}

static int check_matrix(const double *X, i64 T, i64 n, i64 st, i64 sn, const i64 *targets, i64 m) {
    if (!X) return fail(SD_ERR_INVALID, "X is null");
    if (T <= 0 || n <= 0) return fail(SD_ERR_INVALID, "empty matrix (T=%lld, n=%lld)", (long long)T, (long long)n);
    if (n >= ((i64)1 << 31) || T >= ((i64)1 << 31))
        return fail(SD_ERR_UNSUPPORTED, "T and n must be < 2^31");
    if (st <= 0 || sn <= 0) return fail(SD_ERR_INVALID, "strides must be positive (st=%lld, sn=%lld)", (long long)st, (long long)sn);
    if (!((sn == 1 && st >= n) || (st == 1 && sn >= T)))
        return fail(SD_ERR_INVALID, "matrix must be time-major (sn=1, st>=n) or curve-major (st=1, sn>=T)");
    if (m < 0) return fail(SD_ERR_INVALID, "m < 0");
    if (targets == nullptr && m != n) return fail(SD_ERR_INVALID, "targets=NULL requires m == n");
    return SD_OK;
}

// 1 + floor(log2 n): the sorts' steps per key in the work estimates of K10 and K12
static double log2_steps(i64 n) {
    double l = 1.0;
    for (i64 v = n; v > 1; v >>= 1) l += 1.0;
    return l;
}

static bool is_time_major_dense(i64 n, i64 st, i64 sn) { return sn == 1 && st == n; }

// Workspace bytes of the time-major copy that time_major() carves for a matrix in any other layout.
static size_t time_major_bytes(i64 T, i64 n, i64 st, i64 sn) {
    return is_time_major_dense(n, st, sn) ? 0 : align_up((size_t)T * n * 8, 256);
}

// *Y = X when X is time-major dense; otherwise a time-major copy of X carved from cv (sized by time_major_bytes).
static int time_major(const double *X, i64 T, i64 n, i64 st, i64 sn, Carver &cv, hipStream_t s, const double **Y) {
    *Y = X;
    if (is_time_major_dense(n, st, sn)) return SD_OK;
    double *Yw = (double *)cv.take((size_t)T * n * 8);
    if (!Yw) return fail(SD_ERR_WORKSPACE, "workspace too small for the time-major copy");
    int rc = launch_to_time_major(X, T, n, st, sn, Yw, s);
    if (rc) return rc;
    *Y = Yw;
    return SD_OK;
}

// The tail of an entry point of K14 to K17: a workspace below `floor` (named by `floor_name`) is refused; then the time-major
// copy, and launch(Y, ws, ws_bytes, s) with what lies behind it.
template <typename Launch>
static int launch_time_major(const double *X, i64 T, i64 n, i64 st, i64 sn, void *ws, size_t ws_bytes, size_t floor,
                             const char *floor_name, void *stream, Launch launch) {
    if (!ws || ws_bytes < floor) return fail(SD_ERR_WORKSPACE, "workspace below %s", floor_name);
    hipStream_t s = (hipStream_t)stream;
    Carver cv(ws, ws_bytes);
    const double *Y;
    int rc = time_major(X, T, n, st, sn, cv, s, &Y);
    if (rc) return rc;
    const size_t rest = cv.rest();
    return launch(Y, cv.take(rest), rest, s);
}

// The tail of an entry point of K20: launch_time_major with the family's floor, but a floor of 0 bytes (time-major X, nothing
// to carve) takes a null workspace.
template <typename Launch>
static int launch_curve_dist(const double *X, i64 T, i64 n, i64 st, i64 sn, i64 m, int what, void *ws, size_t ws_bytes, void *stream,
                             Launch launch) {
    const size_t floor = sd_curve_sqdist_min_workspace_bytes(T, n, st, sn, m, what);
    if (floor == 0) return launch(X, nullptr, 0, (hipStream_t)stream);
    return launch_time_major(X, T, n, st, sn, ws, ws_bytes, floor, "sd_curve_sqdist_min_workspace_bytes", stream, launch);
}

// The three size functions of a metric depth of curves (K20 to K22), from `sized` (does it take the shape and the number of targets?) and plan(PlanSize),
// its plan of what lies behind the time-major copy: the recommended size holds all targets, the floor one block.
template <typename Plan>
static size_t metric_workspace_bytes(bool sized, i64 T, i64 n, i64 st, i64 sn, i64 m, Plan plan) {
    return sized ? time_major_bytes(T, n, st, sn) + plan(PlanSize::of_rows(m > n ? m : n)).bytes : 0;
}
template <typename Plan>
static size_t metric_min_workspace_bytes(bool sized, i64 T, i64 n, i64 st, i64 sn, i64 m, Plan plan) {
    return sized && m != 0 ? time_major_bytes(T, n, st, sn) + plan(PlanSize::of_rows(1)).bytes : 0;
}
template <typename Plan>
static i64 metric_targets_per_batch(bool sized, i64 T, i64 n, i64 st, i64 sn, size_t ws_bytes, Plan plan) {
    const size_t tm = sized ? time_major_bytes(T, n, st, sn) : 0;
    return sized && ws_bytes >= tm ? plan(PlanSize::of_bytes(ws_bytes - tm)).targets : 0;
}

// wide[i] (two 64-bit limbs) (+)= part[i]: the chunk totals of sd_mbd_counts_wide
__global__ void wide_add_kernel(const u64 *__restrict__ part, i64 count, u64 *__restrict__ wide, int first) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u64 v = part[i];
    if (first) {
        wide[2 * i] = v;
        wide[2 * i + 1] = 0;
    } else {
        const u64 lo = wide[2 * i] + v;
        wide[2 * i + 1] += lo < v ? 1u : 0u;
        wide[2 * i] = lo;
    }
}


}  // namespace sd

using namespace sd;

extern "C" {

int sd_abi_version(void) { return SD_ABI_VERSION; }

const char *sd_last_error(void) { return g_err; }

int sd_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

int sd_device_info(int dev, char *name, int name_len, int *cu_count, size_t *hbm_bytes) {
    hipDeviceProp_t p;
    SD_HIP(hipGetDeviceProperties(&p, dev));
    if (name && name_len > 0) snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName);
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = p.totalGlobalMem;
    return SD_OK;
}

int sd_set_device(int dev) {
    SD_HIP(hipSetDevice(dev));
    return SD_OK;
}

int sd_malloc(void **dptr, size_t bytes) {
    if (!dptr) return fail(SD_ERR_INVALID, "dptr is null");
    SD_HIP(hipMalloc(dptr, bytes ? bytes : 1));
    return SD_OK;
}

int sd_free(void *dptr) {
    if (dptr) SD_HIP(hipFree(dptr));
    return SD_OK;
}

int sd_memcpy_h2d(void *dst, const void *src_host, size_t bytes, void *stream) {
    SD_HIP(hipMemcpyAsync(dst, src_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return SD_OK;
}

int sd_memcpy_d2h(void *dst_host, const void *src, size_t bytes, void *stream) {
    SD_HIP(hipMemcpyAsync(dst_host, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return SD_OK;
}

int sd_memset(void *dst, int value, size_t bytes, void *stream) {
    SD_HIP(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream));
    return SD_OK;
}

int sd_stream_synchronize(void *stream) {
    SD_HIP(hipStreamSynchronize((hipStream_t)stream));
    return SD_OK;
}

// ---------------------------------------------------------------------------
// K1+K2
// ---------------------------------------------------------------------------
size_t sd_mbd_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int J, int algo) {
    if (T <= 0 || n <= 0) return 0;
    size_t b = time_major_bytes(T, n, st, sn);
    b += align_up((size_t)T * 4, 256);   // nan_cnt
    // The sum over the rank routes of the shape, not the planned route's own size: sd_mbd_counts_wide sizes its inner workspace
    // once, for Tc rows, and calls mbd_counts_impl on the last chunk with fewer rows, which may take another route (below 96
    // rows the medium route hands over to the large-n route)
    if (algo == SD_MBD_AUTO || mbd_plan(T, n, m, J, algo, true).route != MbdRoute::Pairwise)
        b += align_up(mbd_rank_routes_workspace_bytes(T, n, J), 256) + 256;
    return b + 1024;
}

// block: the targets are the curves [tbegin, tbegin + m) (sd_mbd_counts_range), whatever m is
static int mbd_counts_impl(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn,
                           const int64_t *targets, bool block, int64_t tbegin, int64_t m, int J, int algo,
                           int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    int rc = check_matrix(X, T, n, st, sn, block ? (const i64 *)1 : targets, m);
    if (rc) return rc;
    if (!targets && (tbegin < 0 || tbegin + m > n))
        return fail(SD_ERR_INVALID, "target block [%lld, %lld) outside [0, %lld)", (long long)tbegin,
                    (long long)(tbegin + m), (long long)n);
    if ((rc = check_count_range(T, n, J))) return rc;
    if (!out) return fail(SD_ERR_INVALID, "out is null");
    if (algo < SD_MBD_AUTO || algo > SD_MBD_RANK) return fail(SD_ERR_INVALID, "unknown algo %d", algo);
    if (m == 0) return SD_OK;
    hipStream_t s = (hipStream_t)stream;
    Carver cv(ws, ws_bytes);
    const double *Y;
    if ((rc = time_major(X, T, n, st, sn, cv, s, &Y))) return rc;
    const MbdPlan plan = mbd_plan(T, n, m, J, algo, !targets && tbegin == 0 && m == n);
    if (plan.route != MbdRoute::Pairwise) {
        void *rws = cv.take(plan.ws_bytes);
        if (plan.ws_bytes && !rws) return fail(SD_ERR_WORKSPACE, "workspace too small for the rank kernels");
        return launch_mbd_rank(plan, Y, T, n, targets, tbegin, m, J, (u64 *)out, rws, s);
    }
    u32 *nan_cnt = (u32 *)cv.take((size_t)T * 4);
    if (!nan_cnt) return fail(SD_ERR_WORKSPACE, "workspace too small (nan counts)");
    if ((rc = launch_nan_count_rows(Y, T, n, nan_cnt, s))) return rc;
    return launch_mbd_pairwise(Y, T, n, targets, tbegin, m, J, nan_cnt, (u64 *)out, s);
}

int sd_mbd_counts(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn,
                  const int64_t *targets, int64_t m, int J, int algo,
                  int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    return mbd_counts_impl(X, T, n, st, sn, targets, false, 0, m, J, algo, out, ws, ws_bytes, stream);
}

int sd_mbd_counts_range(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn,
                        int64_t target_begin, int64_t m, int J, int algo,
                        int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    return mbd_counts_impl(X, T, n, st, sn, nullptr, true, target_begin, m, J, algo, out, ws, ws_bytes, stream);
}

// ---- two-limb totals: T * C(n-1, J) beyond int64 (J >= 4 at n = 10^5) -------------------------------------------
// The kernels accumulate per-timepoint band counts (each < 2^64 by check_count_range's recurrence bound) in 64 bits;
// here the timepoints are cut into chunks whose totals provably fit int64, every chunk runs through the ordinary path,
// and wide_add_kernel adds the chunk's totals into (lo, hi) pairs with carry.
size_t sd_mbd_wide_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int J, int algo) {
    if (T <= 0 || n <= 0 || m < 0 || J < 2) return 0;
    return sd_mbd_workspace_bytes(T, n, st, sn, m, J, algo) + align_up((size_t)m * (J - 1) * 8, 256) + 256;
}

int sd_mbd_counts_wide(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn,
                       const int64_t *targets, int64_t m, int J, int algo,
                       uint64_t *out, void *ws, size_t ws_bytes, void *stream) {
    int rc = check_matrix(X, T, n, st, sn, targets, m);
    if (rc) return rc;
    if (!out) return fail(SD_ERR_INVALID, "out is null");
    if (J < 2 || J > JMAX_HOST) return fail(SD_ERR_INVALID, "J=%d outside [2,%d]", J, JMAX_HOST);
    if (m == 0) return SD_OK;
    // rows per chunk: the largest Tc with Tc * C(n-1, J) < 2^63 (check_count_range's own condition)
    u64 c;
    if (!binom_u64_checked((u64)(n - 1), J, &c))
        return fail(SD_ERR_OVERFLOW, "C(n-1,J) itself overflows 64 bits (n=%lld, J=%d): beyond two-limb totals too",
                    (long long)n, J);
    i64 Tc = c ? (i64)((((u64)1 << 63) - 1) / c) : T;
    if (Tc > T) Tc = T;
    while (Tc > (i64)J && check_count_range(Tc, n, J) != SD_OK) --Tc;      // the check uses max(T, J) rows
    if (Tc < 1 || check_count_range(Tc, n, J) != SD_OK)
        return fail(SD_ERR_OVERFLOW, "J*C(n-1,J) >= 2^63 (n=%lld, J=%d): a single chunk of timepoints does not fit int64",
                    (long long)n, J);
    Carver cv(ws, ws_bytes);
    u64 *part = (u64 *)cv.take((size_t)m * (J - 1) * 8);
    const size_t inner = sd_mbd_workspace_bytes(Tc, n, st, sn, m, J, algo);
    void *iws = cv.take(inner);
    if (!part || !iws) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_mbd_wide_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    const i64 count = m * (J - 1);
    for (i64 t0 = 0; t0 < T; t0 += Tc) {
        const i64 rows = T - t0 < Tc ? T - t0 : Tc;
        // rows [t0, t0 + rows) of either layout: x(t, i) = X[t*st + i*sn]; a curve-major block keeps its curve stride
        if ((rc = mbd_counts_impl(X + t0 * st, rows, n, st, sn, targets, false, 0, m, J, algo, (int64_t *)part, iws, inner, stream)))
            return rc;
        hipLaunchKernelGGL(wide_add_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, part, count,
                           (u64 *)out, t0 == 0 ? 1 : 0);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

int sd_mbd_external_counts(const double *X, int64_t T, int64_t n, const double *Q, int64_t m, int J,
                           int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    if (!X || !Q || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (T <= 0 || n <= 0 || m < 0) return fail(SD_ERR_INVALID, "bad shape (T=%lld, n=%lld, m=%lld)", (long long)T,
                                                (long long)n, (long long)m);
    int rc = check_count_range(T, n + 1, J);
    if (rc) return rc;
    if (m == 0) return SD_OK;
    hipStream_t s = (hipStream_t)stream;
    // bucket structure per row + one look-up per target (O(n + m) per row) when the caller gave the workspace for it
    // (sd_mbd_external_workspace_bytes); the pairwise kernel (O(n m) per row) otherwise
    if (mbd_rank_external_supported(T, n, m, J) && m >= 16 && ws &&
        ws_bytes >= mbd_rank_external_workspace_bytes(T, n, m, J) + 256)
        return launch_mbd_external_rank(X, T, n, Q, m, J, (u64 *)out, ws, ws_bytes, s);
    Carver cv(ws, ws_bytes);
    u32 *nan_cnt = (u32 *)cv.take((size_t)T * 4);
    if (!nan_cnt) return fail(SD_ERR_WORKSPACE, "workspace too small (need T*4 + 256 bytes)");
    if ((rc = launch_nan_count_rows(X, T, n, nan_cnt, s))) return rc;
    return launch_mbd_external(X, T, n, Q, m, J, nan_cnt, (u64 *)out, s);
}

size_t sd_mbd_external_workspace_bytes(int64_t T, int64_t n, int64_t m, int J) {
    if (T <= 0 || n <= 0 || m <= 0) return 0;
    size_t pw = align_up((size_t)T * 4, 256) + 256;                       // pairwise kernel: per-row NaN counts
    size_t rk = mbd_rank_external_workspace_bytes(T, n, m, J);           // 0 where the bucket kernel does not apply
    return (rk ? rk + 256 : 0) > pw ? rk + 256 : pw;
}

int sd_mbd_subset_counts(const double *X, int64_t T, int64_t n, const int32_t *members, int64_t nb, int bs,
                         const int32_t *target, int J, int64_t *out, void *stream) {
    if (!X || !members || !target || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (T <= 0 || n <= 0 || nb < 0 || bs <= 0) return fail(SD_ERR_INVALID, "bad shape");
    int rc = check_count_range(T, bs, J);
    if (rc) return rc;
    if (nb == 0) return SD_OK;
    return launch_mbd_subsets(X, T, n, members, nb, bs, target, J, (u64 *)out, (hipStream_t)stream);
}

int sd_above_below(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn,
                   const int64_t *targets, int64_t m, uint32_t *AB,
                   void *ws, size_t ws_bytes, void *stream) {
    int rc = check_matrix(X, T, n, st, sn, targets, m);
    if (rc) return rc;
    if (!AB) return fail(SD_ERR_INVALID, "AB is null");
    if (m == 0) return SD_OK;
    hipStream_t s = (hipStream_t)stream;
    Carver cv(ws, ws_bytes);
    const double *Y;
    if ((rc = time_major(X, T, n, st, sn, cv, s, &Y))) return rc;
    return launch_above_below(Y, T, n, targets, m, AB, s);
}

// ---------------------------------------------------------------------------
// K3
// ---------------------------------------------------------------------------
size_t sd_bd_strict_j_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int J) {
    if (T <= 0 || n <= 0) return 0;
    return time_major_bytes(T, n, st, sn) + bd_strict_workspace_bytes(T, n, m, J) + 1024;
}

size_t sd_bd_strict_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m) {
    return sd_bd_strict_j_workspace_bytes(T, n, st, sn, m, 2);
}

size_t sd_bd_strict_nanfree_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m) {
    if (T <= 0 || n <= 0) return 0;
    return time_major_bytes(T, n, st, sn) + bd_strict_nanfree_workspace_bytes(T, n, m, 2) + 1024;
}

size_t sd_bd_strict_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int J) {
    if (T <= 0 || n <= 0) return 0;
    return time_major_bytes(T, n, st, sn) + bd_strict_min_workspace_bytes(T, n, m, J) + 1024;
}

int sd_bd_strict_j_counts(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn,
                          const int64_t *targets, int64_t m, int J,
                          int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    int rc = check_matrix(X, T, n, st, sn, targets, m);
    if (rc) return rc;
    if (J < 2 || J > 4) return fail(SD_ERR_UNSUPPORTED, "strict band depth covers J in [2,4], got %d", J);
    if ((rc = check_count_range(1, n, J))) return rc;
    if (!out) return fail(SD_ERR_INVALID, "out is null");
    if (m == 0) return SD_OK;
    hipStream_t s = (hipStream_t)stream;
    Carver cv(ws, ws_bytes);
    const double *Y;
    if ((rc = time_major(X, T, n, st, sn, cv, s, &Y))) return rc;
    size_t need = cv.rest();                                   // batches are sized to what the caller passed
    void *sws = cv.take(need);
    if (!sws || need < bd_strict_launch_floor_bytes(T, n, m, J))
        return fail(SD_ERR_WORKSPACE, "workspace too small for the strict-depth masks (sd_bd_strict_min_workspace_bytes)");
    return launch_bd_strict(Y, T, n, targets, m, J, (u64 *)out, sws, need, s);
}

size_t sd_bd_strict_external_workspace_bytes(int64_t T, int64_t n, int64_t m) {
    if (T <= 0 || n <= 0 || m <= 0) return 0;
    return bd_strict_external_workspace_bytes(T, n, m) + 512;
}

int sd_bd_strict_external_counts(const double *X, int64_t T, int64_t n, const double *Q, int64_t m, int64_t *out, void *ws,
                                 size_t ws_bytes, void *stream) {
    if (!X || !Q || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (T <= 0 || n <= 0 || m < 0) return fail(SD_ERR_INVALID, "bad shape");
    int rc = check_count_range(1, n + 1, 2);
    if (rc) return rc;
    if (m == 0) return SD_OK;
    return launch_bd_strict_external(X, T, n, Q, m, (u64 *)out, ws, ws_bytes, (hipStream_t)stream);
}

size_t sd_bd_strict_subset_workspace_bytes(int64_t T, int64_t nb, int bs) {
    if (T <= 0 || nb <= 0 || bs <= 0) return 0;
    const size_t b = bd_strict_subsets_workspace_bytes(T, nb, bs);
    return b ? b + 512 : 0;
}

int sd_bd_strict_subset_counts(const double *X, int64_t T, int64_t n, const int32_t *members, int64_t nb, int bs,
                               const int32_t *target, int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    if (!X || !members || !target || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (T <= 0 || n <= 0 || nb < 0 || bs <= 0) return fail(SD_ERR_INVALID, "bad shape");
    int rc = check_count_range(1, bs, 2);
    if (rc) return rc;
    if (nb == 0) return SD_OK;
    return launch_bd_strict_subsets(X, T, n, members, nb, bs, target, (u64 *)out, ws, ws_bytes, (hipStream_t)stream);
}

int sd_bd_strict_subset_supported(int64_t T, int bs) { return T > 0 && bs > 0 && bd_strict_subsets_supported(T, bs) ? 1 : 0; }

int sd_bd_strict_counts(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn,
                        const int64_t *targets, int64_t m,
                        int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    return sd_bd_strict_j_counts(X, T, n, st, sn, targets, m, 2, out, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------
// Point clouds (K4, K5, K7, K10, K11).  Every family has a rows, an external and a blocks entry point: each builds its
// PointSel (point_select.h) and calls the family's one function below, which holds the family's checks once.
// ---------------------------------------------------------------------------
static bool rows_form(const PointSel &sel) { return !sel.Q && !sel.members; }

// the blocks entry points' own arguments, checked ahead of the family's (the external ones only have Q)
static int check_blocks(const int32_t *members, int bs) {
    if (!members) return fail(SD_ERR_INVALID, "null pointer");
    if (bs <= 0) return fail(SD_ERR_INVALID, "bad shape");
    return SD_OK;
}

static int check_all_rows(const PointSel &sel, i64 n, i64 m) {
    if (rows_form(sel) && !sel.targets && m != n) return fail(SD_ERR_INVALID, "targets=NULL requires m == n");
    return SD_OK;
}

// ---------------------------------------------------------------------------
// K5
// ---------------------------------------------------------------------------
// (the rows form says "empty point cloud" and has no m < 0 check, the other two say "bad shape": the messages of the
// former per-form entry points, kept as they were; likewise check_simplex's "bad shape" / "m < 0")
static int l1_depth(const double *P, i64 n, int d, const PointSel &sel, i64 m, double *out, void *stream) {
    if (!P || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (n <= 0 || d <= 0 || (m < 0 && !rows_form(sel)))
        return fail(SD_ERR_INVALID, rows_form(sel) ? "empty point cloud" : "bad shape");
    if (d > 64) return fail(SD_ERR_UNSUPPORTED, "l1 depth covers d <= 64");
    int rc = check_all_rows(sel, n, m);
    if (rc) return rc;
    if (m == 0) return SD_OK;
    return launch_l1(P, n, d, sel, m, out, (hipStream_t)stream);
}

int sd_l1_depth(const double *P, int64_t n, int d, const int64_t *targets, int64_t m,
                double *out, void *stream) {
    return l1_depth(P, n, d, select_rows(targets), m, out, stream);
}

int sd_l1_external_depth(const double *P, int64_t n, int d, const double *Q, int64_t m, double *out, void *stream) {
    if (!Q) return fail(SD_ERR_INVALID, "null pointer");
    return l1_depth(P, n, d, select_external(Q), m, out, stream);
}

int sd_l1_subset_depth(const double *P, int64_t n, int d, const int32_t *members, int64_t nb, int bs, double *out,
                       void *stream) {
    int rc = check_blocks(members, bs);
    return rc ? rc : l1_depth(P, n, d, select_blocks(members, bs), nb, out, stream);
}

// ---------------------------------------------------------------------------
// K4
// ---------------------------------------------------------------------------
static int check_simplex(const double *P, i64 n, int d, const PointSel &sel, i64 m, const void *out, bool exhaustive) {
    if (m < 0 && !rows_form(sel)) return fail(SD_ERR_INVALID, sel.members ? "bad shape" : "m < 0");
    if (!P || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (n <= 0) return fail(SD_ERR_INVALID, "empty input");
    if (d < 1 || d > 8) return fail(SD_ERR_UNSUPPORTED, "simplex containment covers d in [1,8], got %d", d);
    int rc = check_all_rows(sel, n, m);
    if (rc) return rc;
    if (exhaustive) {
        const i64 n_others = sel_others_max(sel, n);
        u64 c;
        if (!binom_u64_checked((u64)n_others, d + 1, &c) || (c >> 62))
            return fail(SD_ERR_OVERFLOW, "C(%lld,%d) subsets per target is not enumerable", (long long)n_others, d + 1);
    }
    return SD_OK;
}

// every (d+1)-subset of the others, in any of the three forms
static int simplex_counts(const double *P, i64 n, int d, const PointSel &sel, i64 m, double tol, int64_t *out, void *stream) {
    int rc = check_simplex(P, n, d, sel, m, out, true);
    if (rc) return rc;
    if (m == 0) return SD_OK;
    return launch_pointcloud_simplex(P, n, d, sel, m, tol, -1, 0, (u64 *)out, (hipStream_t)stream);
}

int sd_pointcloud_simplex_counts(const double *P, int64_t n, int d, const int64_t *targets, int64_t m,
                                 double tol, int64_t *out, void *stream) {
    return simplex_counts(P, n, d, select_rows(targets), m, tol, out, stream);
}

int sd_pointcloud_simplex_external_counts(const double *P, int64_t n, int d, const double *Q, int64_t m, double tol,
                                          int64_t *out, void *stream) {
    if (!Q) return fail(SD_ERR_INVALID, "null pointer");
    return simplex_counts(P, n, d, select_external(Q), m, tol, out, stream);
}

int sd_pointcloud_simplex_subset_counts(const double *P, int64_t n, int d, const int32_t *members, int64_t nb, int bs,
                                        double tol, int64_t *out, void *stream) {
    int rc = check_blocks(members, bs);
    return rc ? rc : simplex_counts(P, n, d, select_blocks(members, bs), nb, tol, out, stream);
}

size_t sd_simplex_sampled_workspace_bytes(int64_t n, int64_t T, int d, int64_t samples) {
    return simplex_sampled_workspace_bytes(n, T, d, samples);
}

int sd_pointcloud_simplex_sampled(const double *P, int64_t n, int d, const int64_t *targets, int64_t m,
                                  double tol, int64_t samples, uint64_t seed, int64_t *out, void *ws, size_t ws_bytes,
                                  void *stream) {
    int rc = check_simplex(P, n, d, select_rows(targets), m, out, false);
    if (rc) return rc;
    if (samples <= 0) return fail(SD_ERR_INVALID, "samples must be positive");
    if (n - 1 < d + 1) return fail(SD_ERR_INVALID, "need at least d+2 points");
    if (m == 0) return SD_OK;
    return launch_pointcloud_simplex(P, n, d, select_rows(targets), m, tol, samples, seed, (u64 *)out, (hipStream_t)stream, ws, ws_bytes);
}

int sd_multi_simplex_counts(const double *P, int64_t n, int64_t T, int d, const int64_t *targets, int64_t m,
                            int relax, double tol, int64_t *out, void *stream) {
    int rc = check_simplex(P, n, d, select_rows(targets), m, out, true);
    if (rc) return rc;
    if (T <= 0) return fail(SD_ERR_INVALID, "T <= 0");
    if (m == 0) return SD_OK;
    return launch_multi_simplex(P, n, T, d, targets, m, relax, tol, -1, 0, (u64 *)out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// K6
// ---------------------------------------------------------------------------
size_t sd_multi_band_workspace_bytes(int64_t n, int64_t T, int d) {
    if (n <= 0 || T <= 0 || d <= 0) return 0;
    return multi_band_workspace_bytes(n, T, d);
}

int sd_multi_band_counts(const double *P, int64_t n, int64_t T, int d, const int64_t *targets, int64_t m,
                         int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    if (!P || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (n <= 0 || T <= 0) return fail(SD_ERR_INVALID, "empty input");
    if (d < 1 || d > 8) return fail(SD_ERR_UNSUPPORTED, "componentwise band containment covers d in [1,8], got %d", d);
    if (!targets && m != n) return fail(SD_ERR_INVALID, "targets=NULL requires m == n");
    if (m < 0) return fail(SD_ERR_INVALID, "m < 0");
    int rc = check_count_range(T, n, 2);
    if (rc) return rc;
    if (m == 0) return SD_OK;
    return launch_multi_band(P, n, T, d, targets, m, (u64 *)out, ws, ws_bytes, (hipStream_t)stream);
}

int sd_multi_band_j_counts(const double *P, int64_t n, int64_t T, int d, const int64_t *targets, int64_t m, int J,
                           int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    if (!P || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (n <= 0 || T <= 0) return fail(SD_ERR_INVALID, "empty input");
    if (d < 1 || d > 8) return fail(SD_ERR_UNSUPPORTED, "componentwise band containment covers d in [1,8], got %d", d);
    if (J < 2 || J > 4) return fail(SD_ERR_UNSUPPORTED, "componentwise band containment counts j-subsets for J in [2,4], got %d", J);
    if (!targets && m != n) return fail(SD_ERR_INVALID, "targets=NULL requires m == n");
    if (m < 0) return fail(SD_ERR_INVALID, "m < 0");
    int rc = check_count_range(T, n, J);
    if (rc) return rc;
    if (m == 0) return SD_OK;
    return launch_multi_band_j(P, n, T, d, targets, m, J, (u64 *)out, ws, ws_bytes, (hipStream_t)stream);
}

int sd_multi_simplex_sampled(const double *P, int64_t n, int64_t T, int d, const int64_t *targets, int64_t m,
                             int relax, double tol, int64_t samples, uint64_t seed, int64_t *out, void *ws, size_t ws_bytes,
                             void *stream) {
    int rc = check_simplex(P, n, d, select_rows(targets), m, out, false);
    if (rc) return rc;
    if (T <= 0) return fail(SD_ERR_INVALID, "T <= 0");
    if (samples <= 0) return fail(SD_ERR_INVALID, "samples must be positive");
    if (n - 1 < d + 1) return fail(SD_ERR_INVALID, "need at least d+2 curves");
    if (m == 0) return SD_OK;
    return launch_multi_simplex(P, n, T, d, targets, m, relax, tol, samples, seed, (u64 *)out, (hipStream_t)stream, ws, ws_bytes);
}

// ---------------------------------------------------------------------------
// K7
// ---------------------------------------------------------------------------
static constexpr double OJA_MAX_EVALS = 1e14;   // m * C(others, d): beyond this a call would run for hours

static int oja_volume_sums(const double *P, i64 n, int d, const PointSel &sel, i64 m, double *out, void *stream) {
    const i64 n_others = sel_others_max(sel, n);
    if (!P || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (n <= 0 || m < 0) return fail(SD_ERR_INVALID, "bad shape");
    if (d < 1 || d > 8) return fail(SD_ERR_UNSUPPORTED, "oja volume sums cover d in [1,8], got %d", d);
    if (n_others >= ((i64)1 << 31))                                 // subset indices are 32-bit in the kernel
        return fail(SD_ERR_UNSUPPORTED, "oja volume sums take fewer than 2^31 other points, got %lld", (long long)n_others);
    u64 c;
    if (!binom_u64_checked((u64)(n_others > 0 ? n_others : 0), d, &c) || (c >> 62))
        return fail(SD_ERR_OVERFLOW, "C(%lld,%d) subsets per target is not enumerable", (long long)n_others, d);
    if ((double)m * (double)c > OJA_MAX_EVALS)
        return fail(SD_ERR_UNSUPPORTED, "%lld targets x C(%lld,%d) subsets exceeds the cap of %.0e simplex volumes",
                    (long long)m, (long long)n_others, d, OJA_MAX_EVALS);
    int rc = check_all_rows(sel, n, m);
    if (rc) return rc;
    if (m == 0) return SD_OK;
    return launch_oja(P, n, d, sel, m, out, (hipStream_t)stream);
}

int sd_oja_volume_sums(const double *P, int64_t n, int d, const int64_t *targets, int64_t m, double *out, void *stream) {
    return oja_volume_sums(P, n, d, select_rows(targets), m, out, stream);
}

int sd_oja_external_volume_sums(const double *P, int64_t n, int d, const double *Q, int64_t m, double *out, void *stream) {
    if (!Q) return fail(SD_ERR_INVALID, "null pointer");
    return oja_volume_sums(P, n, d, select_external(Q), m, out, stream);
}

int sd_oja_subset_volume_sums(const double *P, int64_t n, int d, const int32_t *members, int64_t nb, int bs, double *out,
                              void *stream) {
    int rc = check_blocks(members, bs);
    return rc ? rc : oja_volume_sums(P, n, d, select_blocks(members, bs), nb, out, stream);
}

// ---------------------------------------------------------------------------
// K8
// ---------------------------------------------------------------------------
static constexpr double PROB_MAX_EVALS = 1e14;  // pair or (row, column, z) evaluations: beyond this a call runs for hours

int sd_prob_normal_sums(const double *mu, const double *sigma, int64_t n, const int64_t *targets, int64_t m, double *out,
                        void *stream) {
    if (!mu || !sigma || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (n < 0 || m < 0) return fail(SD_ERR_INVALID, "bad shape");
    if (!targets && m != n) return fail(SD_ERR_INVALID, "targets=NULL requires m == n");
    i64 work;
    if (__builtin_mul_overflow((i64)n, (i64)m, &work))
        return fail(SD_ERR_OVERFLOW, "%lld targets x %lld distributions overflows int64", (long long)m, (long long)n);
    if ((double)work > PROB_MAX_EVALS)
        return fail(SD_ERR_UNSUPPORTED, "%lld targets x %lld distributions exceeds the cap of %.0e pairs", (long long)m,
                    (long long)n, PROB_MAX_EVALS);
    if (m == 0) return SD_OK;
    return launch_prob_normal_sums(mu, sigma, n, targets, m, out, (hipStream_t)stream);
}

int sd_prob_poisson_sums(const double *lam, int64_t T, int64_t n, int64_t lim, const int64_t *targets, int64_t m, double *out,
                         void *stream) {
    if (!lam || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (T < 0 || n < 0 || m < 0) return fail(SD_ERR_INVALID, "bad shape");
    if (!targets && m != n) return fail(SD_ERR_INVALID, "targets=NULL requires m == n");
    i64 work = 0, tn;
    if (__builtin_mul_overflow((i64)T, (i64)n, &tn) || (lim > 1 && __builtin_mul_overflow(tn, (i64)(lim - 1), &work)))
        return fail(SD_ERR_OVERFLOW, "%lld rows x %lld curves x lim %lld overflows int64", (long long)T, (long long)n,
                    (long long)lim);
    if ((double)work > PROB_MAX_EVALS)
        return fail(SD_ERR_UNSUPPORTED, "%lld rows x %lld curves x lim %lld exceeds the cap of %.0e evaluations", (long long)T,
                    (long long)n, (long long)lim, PROB_MAX_EVALS);
    if (m == 0) return SD_OK;
    return launch_prob_poisson_sums(lam, T, n, lim, targets, m, out, (hipStream_t)stream);
}

int sd_prob_band_sums(const double *mu, const double *var, int64_t T, int64_t n, const int64_t *targets, int64_t m,
                      const int32_t *members, int bs, int relax, double *out, void *stream) {
    if (!mu || !var || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (T < 0 || n < 0 || m < 0 || (members && bs < 0)) return fail(SD_ERR_INVALID, "bad shape");
    if (!targets && m != n) return fail(SD_ERR_INVALID, "targets=NULL requires m == n");
    const i64 W = members ? (i64)bs : n;                           // positions per target
    i64 pairs = 0, work = 0;
    if (W > 1 && (__builtin_mul_overflow(W, W - 1, &pairs) || __builtin_mul_overflow(pairs / 2, (i64)T, &work) ||
                  __builtin_mul_overflow(work, (i64)m, &work)))
        return fail(SD_ERR_OVERFLOW, "%lld targets x %lld pairs x %lld timepoints overflows int64", (long long)m,
                    (long long)(W / 2) * (long long)(W - 1), (long long)T);
    if ((double)work > PROB_MAX_EVALS)
        return fail(SD_ERR_UNSUPPORTED, "%lld targets x %lld positions x %lld timepoints exceeds the cap of %.0e pair "
                    "evaluations", (long long)m, (long long)W, (long long)T, PROB_MAX_EVALS);
    if (m == 0) return SD_OK;
    return launch_prob_band_sums(mu, var, T, n, targets, m, members, bs, relax, out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// K10
// ---------------------------------------------------------------------------
static constexpr double HS_MAX_WORK = 1e14;     // projections and comparisons: beyond this a call would run for hours

// shape checks shared by the four entry points; `others` = points a target is compared with, work = the call's estimate
static int check_halfspace(const double *P, i64 n, int d, const double *U, i64 k, i64 m, const void *out, i64 others,
                           double work) {
    if (!P || !U || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (n < 1 || d < 1 || k < 1 || m < 0) return fail(SD_ERR_INVALID, "bad shape (n=%lld, d=%d, k=%lld, m=%lld)", (long long)n,
                                                       d, (long long)k, (long long)m);
    if (d > 8) return fail(SD_ERR_UNSUPPORTED, "halfspace counts cover d in [1,8], got %d", d);
    if (n >= ((i64)1 << 31) || others >= ((i64)1 << 31))          // counts and indices are 32-bit in the kernels
        return fail(SD_ERR_UNSUPPORTED, "halfspace counts take fewer than 2^31 points, got %lld", (long long)n);
    if (k >= ((i64)1 << 31)) return fail(SD_ERR_UNSUPPORTED, "halfspace counts take fewer than 2^31 directions");
    if (work > HS_MAX_WORK)
        return fail(SD_ERR_UNSUPPORTED, "%.3g projections and comparisons exceed the cap of %.0e", work, HS_MAX_WORK);
    return SD_OK;
}

size_t sd_halfspace_workspace_bytes(int64_t n, int d, int64_t k) {
    if (n < 1 || d < 1 || k < 1 || n >= ((i64)1 << 31)) return 0;
    return halfspace_workspace_bytes(n, k);
}

size_t sd_halfspace_min_workspace_bytes(int64_t n, int d, int64_t k) {
    if (n < 1 || d < 1 || k < 1 || n >= ((i64)1 << 31)) return 0;
    return halfspace_min_workspace_bytes(n);
}

int sd_halfspace_counts(const double *P, int64_t n, int d, const double *U, int64_t k, const int64_t *targets, int64_t m,
                        int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    const double logn = log2_steps(n);
    int rc = check_halfspace(P, n, d, U, k, m, out, n, (double)k * (double)n * ((double)d + logn));
    if (rc) return rc;
    if (!targets && m != n) return fail(SD_ERR_INVALID, "targets=NULL requires m == n");
    if (m == 0) return SD_OK;
    return launch_halfspace_counts(P, n, d, U, k, targets, m, out, ws, ws_bytes, (hipStream_t)stream);
}

static int halfspace_pairwise(const double *P, i64 n, int d, const double *U, i64 k, const PointSel &sel, i64 m, int64_t *out,
                              void *stream) {
    int rc = check_halfspace(P, n, d, U, k, m, out, sel_others_max(sel, n) + 1,
                             (double)m * (double)sel_cnt_max(sel, n) * (double)k * (double)d);
    if (rc) return rc;
    if ((rc = check_all_rows(sel, n, m))) return rc;
    if (m == 0) return SD_OK;
    return launch_halfspace_pairwise(P, n, d, U, k, sel, m, out, (hipStream_t)stream);
}

int sd_halfspace_pairwise_counts(const double *P, int64_t n, int d, const double *U, int64_t k, const int64_t *targets,
                                 int64_t m, int64_t *out, void *stream) {
    return halfspace_pairwise(P, n, d, U, k, select_rows(targets), m, out, stream);
}

int sd_halfspace_external_counts(const double *P, int64_t n, int d, const double *U, int64_t k, const double *Q, int64_t m,
                                 int64_t *out, void *stream) {
    if (!Q) return fail(SD_ERR_INVALID, "null pointer");
    return halfspace_pairwise(P, n, d, U, k, select_external(Q), m, out, stream);
}

int sd_halfspace_subset_counts(const double *P, int64_t n, int d, const double *U, int64_t k, const int32_t *members,
                               int64_t nb, int bs, int64_t *out, void *stream) {
    int rc = check_blocks(members, bs);
    return rc ? rc : halfspace_pairwise(P, n, d, U, k, select_blocks(members, bs), nb, out, stream);
}

// ---------------------------------------------------------------------------
// K11
// ---------------------------------------------------------------------------
static int halfspace2_counts(const double *P, i64 n, const PointSel &sel, i64 m, int algo, int64_t *out, void *stream) {
    const i64 cnt_max = sel_cnt_max(sel, n);                      // the largest sample in P
    if (!P || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (n < 1 || m < 0) return fail(SD_ERR_INVALID, "bad shape (n=%lld, m=%lld)", (long long)n, (long long)m);
    if (algo < 0 || algo > 2) return fail(SD_ERR_INVALID, "algo=%d outside 0 (auto), 1 (sweep), 2 (pairwise)", algo);
    if (n >= ((i64)1 << 31) || sel_others_max(sel, n) + 1 >= ((i64)1 << 31))   // counts and indices are 32-bit in the kernels
        return fail(SD_ERR_UNSUPPORTED, "exact halfspace counts take fewer than 2^31 points, got %lld", (long long)n);
    const int route = halfspace2_route(algo, cnt_max);              // the route that runs (1 sweep, 2 pairwise)
    if (route == 0)
        return fail(SD_ERR_UNSUPPORTED, "the sweep holds samples of up to %lld points, got %lld (algo 0 or 2 takes them)",
                    (long long)HX_SWEEP_CAPACITY, (long long)cnt_max);
    const double work = halfspace2_work(route, m, cnt_max);
    if (work > HS_MAX_WORK)
        return fail(SD_ERR_UNSUPPORTED, "%.3g predicate evaluations exceed the cap of %.0e", work, HS_MAX_WORK);
    int rc = check_all_rows(sel, n, m);
    if (rc) return rc;
    if (m == 0) return SD_OK;
    return launch_halfspace2(P, n, sel, m, route, out, (hipStream_t)stream);
}

int sd_halfspace2_counts(const double *P, int64_t n, const int64_t *targets, int64_t m, int algo, int64_t *out,
                         void *stream) {
    return halfspace2_counts(P, n, select_rows(targets), m, algo, out, stream);
}

int sd_halfspace2_external_counts(const double *P, int64_t n, const double *Q, int64_t m, int algo, int64_t *out,
                                  void *stream) {
    if (!Q) return fail(SD_ERR_INVALID, "null pointer");
    return halfspace2_counts(P, n, select_external(Q), m, algo, out, stream);
}

int sd_halfspace2_subset_counts(const double *P, int64_t n, const int32_t *members, int64_t nb, int bs, int algo,
                                int64_t *out, void *stream) {
    int rc = check_blocks(members, bs);
    return rc ? rc : halfspace2_counts(P, n, select_blocks(members, bs), nb, algo, out, stream);
}

// ---------------------------------------------------------------------------
// K12
// ---------------------------------------------------------------------------
// shape checks shared by the three entry points; `sample` = the largest sample of the call, work = the call's estimate
static int check_projection(const double *P, i64 n, int d, const double *U, i64 k, i64 m, const void *out, i64 sample,
                            double work) {
    if (!P || !U || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (n < 1 || d < 1 || k < 1 || m < 0) return fail(SD_ERR_INVALID, "bad shape (n=%lld, d=%d, k=%lld, m=%lld)", (long long)n,
                                                       d, (long long)k, (long long)m);
    if (d > 8) return fail(SD_ERR_UNSUPPORTED, "projection outlyingness covers d in [1,8], got %d", d);
    if (n >= ((i64)1 << 31) || sample >= ((i64)1 << 31))          // the sort's indices are 32-bit
        return fail(SD_ERR_UNSUPPORTED, "projection outlyingness takes fewer than 2^31 points, got %lld", (long long)n);
    if (k >= ((i64)1 << 31)) return fail(SD_ERR_UNSUPPORTED, "projection outlyingness takes fewer than 2^31 directions");
    if (work > HS_MAX_WORK)
        return fail(SD_ERR_UNSUPPORTED, "%.3g projections and comparisons exceed the cap of %.0e", work, HS_MAX_WORK);
    return SD_OK;
}

size_t sd_projection_workspace_bytes(int64_t n, int d, int64_t k) {
    if (n < 1 || d < 1 || k < 1 || n >= ((i64)1 << 31)) return 0;
    return projection_workspace_bytes(n, k);
}

size_t sd_projection_min_workspace_bytes(int64_t n, int d, int64_t k) {
    if (n < 1 || d < 1 || k < 1 || n >= ((i64)1 << 31)) return 0;
    return projection_min_workspace_bytes(n);
}

// rows and external form: sort per chunk of directions, then m k evaluations (external: with a selection each)
static int projection_sorted(const double *P, i64 n, int d, const double *U, i64 k, const PointSel &sel, i64 m, double *out,
                             void *ws, size_t ws_bytes, void *stream) {
    const double logn = log2_steps(n);
    int rc = check_projection(P, n, d, U, k, m, out, sel_others_max(sel, n) + 1,
                              (double)k * (double)n * ((double)d + logn) +
                                  (double)m * (double)k * ((double)d + (sel.Q ? 3.0 * logn : 0.0)));
    if (rc) return rc;
    if ((rc = check_all_rows(sel, n, m))) return rc;
    if (m == 0) return SD_OK;
    return launch_projection_sorted(P, n, d, U, k, sel, m, out, ws, ws_bytes, (hipStream_t)stream);
}

int sd_projection_outlyingness(const double *P, int64_t n, int d, const double *U, int64_t k, const int64_t *targets,
                               int64_t m, double *out, void *ws, size_t ws_bytes, void *stream) {
    return projection_sorted(P, n, d, U, k, select_rows(targets), m, out, ws, ws_bytes, stream);
}

int sd_projection_external_outlyingness(const double *P, int64_t n, int d, const double *U, int64_t k, const double *Q,
                                        int64_t m, double *out, void *ws, size_t ws_bytes, void *stream) {
    if (!Q) return fail(SD_ERR_INVALID, "null pointer");
    return projection_sorted(P, n, d, U, k, select_external(Q), m, out, ws, ws_bytes, stream);
}

int sd_projection_subset_outlyingness(const double *P, int64_t n, int d, const double *U, int64_t k, const int32_t *members,
                                      int64_t nb, int bs, double *out, void *stream) {
    int rc = check_blocks(members, bs);
    if (rc) return rc;
    const double logb = log2_steps(bs);
    rc = check_projection(P, n, d, U, k, nb, out, bs, (double)nb * (double)k * (double)bs * ((double)d + logb * logb));
    if (rc) return rc;
    if (bs > PD_MAX_BLOCK)
        return fail(SD_ERR_UNSUPPORTED, "projection outlyingness takes blocks of at most %d members, got %d", PD_MAX_BLOCK, bs);
    if (nb == 0) return SD_OK;
    return launch_projection_blocks(P, n, d, U, k, select_blocks(members, bs), nb, out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// K13
// ---------------------------------------------------------------------------
static int simplicial2_counts(const double *P, i64 n, const PointSel &sel, i64 m, int algo, int64_t *out, void *stream) {
    const i64 others_max = sel_others_max(sel, n);                // the most vectors a target has
    if (!P || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (n < 1 || m < 0) return fail(SD_ERR_INVALID, "bad shape (n=%lld, m=%lld)", (long long)n, (long long)m);
    if (algo < 0 || algo > 2) return fail(SD_ERR_INVALID, "algo=%d outside 0 (auto), 1 (sweep), 2 (pairwise)", algo);
    if (n >= ((i64)1 << 31) || others_max + 1 >= ((i64)1 << 31))    // counts and indices are 32-bit in the kernels
        return fail(SD_ERR_UNSUPPORTED, "exact simplicial counts take fewer than 2^31 points, got %lld", (long long)n);
    const int route = simplicial2_route(algo, others_max);          // the route that runs (1 sweep, 2 pairwise)
    if (route == 0)
        return fail(SD_ERR_UNSUPPORTED, "the sweep holds up to %lld other points, got %lld (algo 0 or 2 takes them)",
                    (long long)SX_SWEEP_CAPACITY, (long long)others_max);
    if (others_max > simplicial2_max_others())
        return fail(SD_ERR_UNSUPPORTED, "C(%lld, 3) triples overflow int64: at most %lld other points", (long long)others_max,
                    (long long)simplicial2_max_others());
    const double work = simplicial2_work(route, m, others_max);
    if (work > HS_MAX_WORK)
        return fail(SD_ERR_UNSUPPORTED, "%.3g predicate evaluations exceed the cap of %.0e", work, HS_MAX_WORK);
    int rc = check_all_rows(sel, n, m);
    if (rc) return rc;
    if (m == 0) return SD_OK;
    return launch_simplicial2(P, n, sel, m, route, out, (hipStream_t)stream);
}

int sd_simplicial2_counts(const double *P, int64_t n, const int64_t *targets, int64_t m, int algo, int64_t *out,
                          void *stream) {
    return simplicial2_counts(P, n, select_rows(targets), m, algo, out, stream);
}

int sd_simplicial2_external_counts(const double *P, int64_t n, const double *Q, int64_t m, int algo, int64_t *out,
                                   void *stream) {
    if (!Q) return fail(SD_ERR_INVALID, "null pointer");
    return simplicial2_counts(P, n, select_external(Q), m, algo, out, stream);
}

int sd_simplicial2_subset_counts(const double *P, int64_t n, const int32_t *members, int64_t nb, int bs, int algo,
                                 int64_t *out, void *stream) {
    int rc = check_blocks(members, bs);
    return rc ? rc : simplicial2_counts(P, n, select_blocks(members, bs), nb, algo, out, stream);
}

// ---------------------------------------------------------------------------
// K14, K15, K17: the curve depths on the pair image (curve_routes.h), and K16
// ---------------------------------------------------------------------------
// The refusals that restate curve_route, in the family's words.  Each family keeps its own order of checks.
static const char *const RD_ALGO_NAMES = "0 (auto), 1 (image), 2 (sort)", *const TVD_ALGO_NAMES = "0 (auto), 1 (LDS), 2 (pairwise)";

static int refuse_algo(int algo, const char *names) {
    return algo < 0 || algo > 2 ? fail(SD_ERR_INVALID, "algo=%d outside %s", algo, names) : SD_OK;
}

static int refuse_curves(i64 n, const char *family_takes) {
    return n >= ((i64)1 << 31) ? fail(SD_ERR_UNSUPPORTED, "%s fewer than 2^31 curves, got %lld", family_takes, (long long)n) : SD_OK;
}

static int refuse_route1(int algo, i64 n, const char *route1) {
    if (algo != 1 || n <= RD_IMAGE_MAX_N) return SD_OK;
    return fail(SD_ERR_UNSUPPORTED, "the %s route holds up to %lld curves, got %lld (algo 0 or 2 takes them)", route1,
                (long long)RD_IMAGE_MAX_N, (long long)n);
}

// ---- K14 ----
size_t sd_rank_depth_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo) {
    (void)m;
    const int route = curve_route(algo, T, n);
    return route ? time_major_bytes(T, n, st, sn) + pair_image_plan(T, n, route, PlanSize::of_rows(T)).bytes : 0;
}

size_t sd_rank_depth_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo) {
    (void)m;
    const int route = curve_route(algo, T, n);
    return route ? time_major_bytes(T, n, st, sn) + pair_image_plan(T, n, route, PlanSize::of_rows(1)).bytes : 0;
}

int64_t sd_rank_depth_rows_per_batch(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo, size_t ws_bytes) {
    (void)m;
    const int route = curve_route(algo, T, n);
    const size_t tm = route ? time_major_bytes(T, n, st, sn) : 0;
    return route && ws_bytes >= tm ? pair_image_plan(T, n, route, PlanSize::of_bytes(ws_bytes - tm)).rows : 0;
}

int sd_rank_depth_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m,
                       int algo, int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    if (!X || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (T < 1 || n < 2) return fail(SD_ERR_INVALID, "bad shape (T=%lld, n=%lld): at least one timepoint and two curves",
                                    (long long)T, (long long)n);
    int rc;
    if ((rc = refuse_algo(algo, RD_ALGO_NAMES)) || (rc = refuse_curves(n, "rank depths take")) ||
        (rc = refuse_route1(algo, n, "image")) || (rc = check_matrix(X, T, n, st, sn, targets, m)))
        return rc;
    if (m == 0) return SD_OK;
    const int route = curve_route(algo, T, n);
    return launch_time_major(X, T, n, st, sn, ws, ws_bytes, sd_rank_depth_min_workspace_bytes(T, n, st, sn, m, algo),
                             "sd_rank_depth_min_workspace_bytes", stream, [&](const double *Y, void *w, size_t bytes, hipStream_t s) {
                                 return launch_rank_depth_sums(Y, T, n, targets, m, route, out, w, bytes, s);
                             });
}

// ---- K15 ----
// the route of a shape the extremal depth takes, 0 otherwise
static int curve_route_k15(int algo, i64 T, i64 n) { return T > EX_MAX_T ? 0 : curve_route(algo, T, n); }

size_t sd_extremal_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo) {
    (void)m;
    const int route = curve_route_k15(algo, T, n);
    return route ? time_major_bytes(T, n, st, sn) + extremal_plan(T, n, route, PlanSize::of_rows(T)).bytes : 0;
}

size_t sd_extremal_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo) {
    (void)m;
    const int route = curve_route_k15(algo, T, n);
    return route ? time_major_bytes(T, n, st, sn) + extremal_plan(T, n, route, PlanSize::of_rows(1)).bytes : 0;
}

int sd_extremal_counts(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m,
                       int algo, int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    if (!X || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (T < 1 || n < 2) return fail(SD_ERR_INVALID, "bad shape (T=%lld, n=%lld): at least one timepoint and two curves",
                                    (long long)T, (long long)n);
    int rc = refuse_algo(algo, RD_ALGO_NAMES);
    if (rc) return rc;
    if (T > EX_MAX_T)
        return fail(SD_ERR_UNSUPPORTED, "extremal depth sorts up to %lld timepoints per curve, got %lld", (long long)EX_MAX_T,
                    (long long)T);
    if ((rc = refuse_curves(n, "extremal depth takes")) || (rc = refuse_route1(algo, n, "image"))) return rc;
    const double walk = (double)n * (double)m * (double)T;         // every pair undecided by its head, to the last entry
    if (walk > HS_MAX_WORK)
        return fail(SD_ERR_UNSUPPORTED, "%.3g entry comparisons in the worst case exceed the cap of %.0e", walk, HS_MAX_WORK);
    if ((rc = check_matrix(X, T, n, st, sn, targets, m))) return rc;
    if (m == 0) return SD_OK;
    const int route = curve_route_k15(algo, T, n);
    return launch_time_major(X, T, n, st, sn, ws, ws_bytes, sd_extremal_min_workspace_bytes(T, n, st, sn, m, algo),
                             "sd_extremal_min_workspace_bytes", stream, [&](const double *Y, void *w, size_t bytes, hipStream_t s) {
                                 return launch_extremal_counts(Y, T, n, targets, m, route, out, w, bytes, s);
                             });
}

// ---- K16 ----
int64_t sd_central_regions_row_capacity(void) { return CR_ROW_CAPACITY; }

size_t sd_central_regions_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int L) {
    if (T < 1 || n < 1 || T >= ((i64)1 << 31) || n >= ((i64)1 << 31) || L < 1 || L > 8) return 0;
    return time_major_bytes(T, n, st, sn) + central_regions_workspace_bytes(T, n, L);
}

int sd_central_regions(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const uint8_t *level, int L, int box,
                       double factor, double *env, double *fence, int32_t *outside, double *whisker, void *ws, size_t ws_bytes,
                       void *stream) {
    if (!X || !level || !env) return fail(SD_ERR_INVALID, "null pointer (X, level and env are required)");
    if (T < 1 || n < 1) return fail(SD_ERR_INVALID, "bad shape (T=%lld, n=%lld): at least one timepoint and one curve",
                                    (long long)T, (long long)n);
    if (L < 1 || L > 8) return fail(SD_ERR_INVALID, "L=%d outside [1,8]", L);
    if (box < -1 || box >= L) return fail(SD_ERR_INVALID, "box=%d outside [-1,%d)", box, L);
    if (!(factor >= 0.0) || factor > 1.79769313486231570815e308)
        return fail(SD_ERR_INVALID, "the fence factor must be finite and not negative, got %g", factor);
    if (box < 0 && (fence || outside || whisker))
        return fail(SD_ERR_INVALID, "box=-1 asks for the envelopes only: fence, outside and whisker must be null");
    int rc = check_matrix(X, T, n, st, sn, nullptr, n);
    if (rc) return rc;
    return launch_time_major(X, T, n, st, sn, ws, ws_bytes, sd_central_regions_workspace_bytes(T, n, st, sn, L),
                             "sd_central_regions_workspace_bytes", stream, [&](const double *Y, void *w, size_t bytes, hipStream_t s) {
                                 return launch_central_regions(Y, T, n, level, L, box, factor, env, fence, outside, whisker, w, bytes, s);
                             });
}

// ---- K17 ----
// the route (1 LDS, 2 pairwise) of a shape and a number of targets the total variation depth takes, 0 otherwise
static int curve_route_k17(int algo, i64 T, i64 n, i64 m) { return m < 0 || T >= ((i64)1 << 31) ? 0 : curve_route(algo, T, n); }

size_t sd_tvd_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo) {
    const int route = curve_route_k17(algo, T, n, m);
    return route ? time_major_bytes(T, n, st, sn) + tvd_plan(T, n, m, route, PlanSize::of_rows(T)).bytes : 0;
}

size_t sd_tvd_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo) {
    const int route = curve_route_k17(algo, T, n, m);
    return route ? time_major_bytes(T, n, st, sn) + tvd_plan(T, n, m, route, PlanSize::of_rows(1)).bytes : 0;
}

int64_t sd_tvd_rows_per_batch(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int algo, size_t ws_bytes) {
    const int route = curve_route_k17(algo, T, n, m);
    const size_t tm = route ? time_major_bytes(T, n, st, sn) : 0;
    return route && ws_bytes >= tm ? tvd_plan(T, n, m, route, PlanSize::of_bytes(ws_bytes - tm)).rows : 0;
}

int sd_tvd_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m, int algo,
                int64_t *sd_sum, double *shape, uint32_t *counts, void *ws, size_t ws_bytes, void *stream) {
    if (!X || !sd_sum || !shape) return fail(SD_ERR_INVALID, "null pointer (X, sd_sum and shape are required)");
    if (T < 1 || n < 1) return fail(SD_ERR_INVALID, "bad shape (T=%lld, n=%lld): at least one timepoint", (long long)T, (long long)n);
    int rc = refuse_algo(algo, TVD_ALGO_NAMES);
    if (rc) return rc;
    if (n < 2) return fail(SD_ERR_UNSUPPORTED, "the total variation depth needs at least two curves, got %lld", (long long)n);
    if ((rc = refuse_route1(algo, n, "LDS")) || (rc = check_matrix(X, T, n, st, sn, targets, m))) return rc;
    const int route = curve_route_k17(algo, T, n, m);
    const double work = (double)n * (double)m * (double)T;         // comparisons of the pairwise route
    if (route == 2 && work > HS_MAX_WORK)
        return fail(SD_ERR_UNSUPPORTED, "%.3g comparisons of the pairwise route exceed the cap of %.0e", work, HS_MAX_WORK);
    if (m == 0) return SD_OK;
    return launch_time_major(X, T, n, st, sn, ws, ws_bytes, sd_tvd_min_workspace_bytes(T, n, st, sn, m, algo),
                             "sd_tvd_min_workspace_bytes", stream, [&](const double *Y, void *w, size_t bytes, hipStream_t s) {
                                 return launch_tvd_sums(Y, T, n, targets, m, route, sd_sum, shape, counts, w, bytes, s);
                             });
}

// ---- K20 ----
// does the family take the shape, the number of targets and `what` (CD_WHAT_*)?
static bool curve_dist_sized(i64 T, i64 n, i64 m, int what) {
    return T >= 1 && n >= 2 && m >= 0 && T < ((i64)1 << 31) && n < ((i64)1 << 31) && what >= CD_WHAT_SQDIST && what <= CD_WHAT_SELECT;
}

size_t sd_curve_sqdist_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int what) {
    return metric_workspace_bytes(curve_dist_sized(T, n, m, what), T, n, st, sn, m, [&](PlanSize z) { return curve_dist_plan(what, n, m, z); });
}

size_t sd_curve_sqdist_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int what) {
    return metric_min_workspace_bytes(curve_dist_sized(T, n, m, what), T, n, st, sn, m, [&](PlanSize z) { return curve_dist_plan(what, n, m, z); });
}

int64_t sd_curve_sqdist_targets_per_batch(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, int what, size_t ws_bytes) {
    return metric_targets_per_batch(curve_dist_sized(T, n, m, what), T, n, st, sn, ws_bytes, [&](PlanSize z) { return curve_dist_plan(what, n, m, z); });
}

// the refusals of K20's and K21's entry points, in sd_tvd_sums' order: pointers, shape, size, matrix, work
// (the columns of Q: any m >= 0)
static int check_curve_dist(const double *X, i64 T, i64 n, i64 st, i64 sn, CurveSel sel, i64 m, const void *out, double passes) {
    if (!X || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (T < 1 || n < 1) return fail(SD_ERR_INVALID, "bad shape (T=%lld, n=%lld): at least one timepoint", (long long)T, (long long)n);
    if (n < 2) return fail(SD_ERR_UNSUPPORTED, "distances between curves need at least two curves, got %lld", (long long)n);
    int rc = sel.Q ? check_matrix(X, T, n, st, sn, nullptr, n) : check_matrix(X, T, n, st, sn, sel.targets, m);
    if (rc) return rc;
    if (m < 0) return fail(SD_ERR_INVALID, "m < 0");
    const double work = passes * (double)n * (double)m * (double)T;
    if (work > HS_MAX_WORK) return fail(SD_ERR_UNSUPPORTED, "%.3g pair-timepoints exceed the cap of %.0e", work, HS_MAX_WORK);
    return SD_OK;
}

static int check_bandwidth_factor(double g) {
    return g > 0.0 && g <= 1.79769313486231570815e308 ? SD_OK
                                                      : fail(SD_ERR_INVALID, "g = 1 / (2 h^2) must be positive and finite, got %g", g);
}

// Each pair of entry points, sample targets and columns of Q, is one function of the selector.
static int curve_sqdist_of(const double *X, i64 T, i64 n, i64 st, i64 sn, CurveSel sel, i64 m, double *out, void *ws, size_t ws_bytes,
                           void *stream) {
    int rc = check_curve_dist(X, T, n, st, sn, sel, m, out, 1.0);
    if (rc || m == 0) return rc;
    return launch_curve_dist(X, T, n, st, sn, m, CD_WHAT_SQDIST, ws, ws_bytes, stream,
                             [&](const double *Y, void *, size_t, hipStream_t s) { return launch_curve_sqdist(Y, T, n, sel, m, out, s); });
}

int sd_curve_sqdist(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m, double *out,
                    void *ws, size_t ws_bytes, void *stream) {
    return curve_sqdist_of(X, T, n, st, sn, select_sample(targets), m, out, ws, ws_bytes, stream);
}

int sd_curve_sqdist_external(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *Q, int64_t m, double *out,
                             void *ws, size_t ws_bytes, void *stream) {
    if (!Q) return fail(SD_ERR_INVALID, "null pointer");
    return curve_sqdist_of(X, T, n, st, sn, select_columns(Q), m, out, ws, ws_bytes, stream);
}

int sd_curve_sqdist_select(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, int64_t k, double *out, void *ws,
                           size_t ws_bytes, void *stream) {
    int rc = check_curve_dist(X, T, n, st, sn, select_sample(nullptr), n, out, 3.0);                // six passes over half the pairs
    if (rc) return rc;
    const i64 N = n * (n - 1) / 2;
    if (k < 1 || k > N) return fail(SD_ERR_INVALID, "k=%lld outside [1, %lld], the pairs of %lld curves", (long long)k, (long long)N, (long long)n);
    return launch_curve_dist(X, T, n, st, sn, n, CD_WHAT_SELECT, ws, ws_bytes, stream, [&](const double *Y, void *w, size_t bytes, hipStream_t s) {
        return launch_curve_sqdist_select(Y, T, n, (u64)k, out, w, bytes, s);
    });
}

static int hmodal_sums_of(const double *X, i64 T, i64 n, i64 st, i64 sn, CurveSel sel, i64 m, double g, double *out, void *ws,
                          size_t ws_bytes, void *stream) {
    int rc = check_curve_dist(X, T, n, st, sn, sel, m, out, 1.0);
    if (rc || (rc = check_bandwidth_factor(g)) || m == 0) return rc;
    return launch_curve_dist(X, T, n, st, sn, m, CD_WHAT_HMODAL, ws, ws_bytes, stream, [&](const double *Y, void *w, size_t bytes, hipStream_t s) {
        return launch_hmodal_sums(Y, T, n, sel, m, g, out, w, bytes, s);
    });
}

int sd_hmodal_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m, double g,
                   double *out, void *ws, size_t ws_bytes, void *stream) {
    return hmodal_sums_of(X, T, n, st, sn, select_sample(targets), m, g, out, ws, ws_bytes, stream);
}

int sd_hmodal_external_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *Q, int64_t m, double g,
                            double *out, void *ws, size_t ws_bytes, void *stream) {
    if (!Q) return fail(SD_ERR_INVALID, "null pointer");
    return hmodal_sums_of(X, T, n, st, sn, select_columns(Q), m, g, out, ws, ws_bytes, stream);
}

// ---- K21 ----
static bool spatial_sized(i64 T, i64 n, i64 m) {
    return T >= 1 && n >= 2 && m >= 0 && T < ((i64)1 << 31) && n < ((i64)1 << 31);
}

size_t sd_spatial_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m) {
    return metric_workspace_bytes(spatial_sized(T, n, m), T, n, st, sn, m, [&](PlanSize z) { return spatial_plan(T, n, m, z); });
}

size_t sd_spatial_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m) {
    return metric_min_workspace_bytes(spatial_sized(T, n, m), T, n, st, sn, m, [&](PlanSize z) { return spatial_plan(T, n, m, z); });
}

int64_t sd_spatial_targets_per_batch(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, size_t ws_bytes) {
    return metric_targets_per_batch(spatial_sized(T, n, m), T, n, st, sn, ws_bytes, [&](PlanSize z) { return spatial_plan(T, n, m, z); });
}

int64_t sd_spatial_time_tile(int64_t T, int64_t targets, void *stream) {
    if (T < 1 || targets < 1) return 0;
    return spatial_time_tile(T, targets, stream_cus((hipStream_t)stream));
}

// K20's refusals in K20's order; the two passes count 2 n m T pair-timepoints
static int spatial_sums_of(const double *X, i64 T, i64 n, i64 st, i64 sn, CurveSel sel, i64 m, double *out, double *field, void *ws,
                           size_t ws_bytes, void *stream) {
    int rc = check_curve_dist(X, T, n, st, sn, sel, m, out, 2.0);
    if (rc || m == 0) return rc;
    return launch_time_major(X, T, n, st, sn, ws, ws_bytes, sd_spatial_min_workspace_bytes(T, n, st, sn, m),
                             "sd_spatial_min_workspace_bytes", stream, [&](const double *Y, void *w, size_t bytes, hipStream_t s) {
                                 return launch_spatial_sums(Y, T, n, sel, m, out, field, w, bytes, s);
                             });
}

int sd_spatial_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m, double *out,
                    double *field, void *ws, size_t ws_bytes, void *stream) {
    return spatial_sums_of(X, T, n, st, sn, select_sample(targets), m, out, field, ws, ws_bytes, stream);
}

int sd_spatial_external_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *Q, int64_t m, double *out,
                             double *field, void *ws, size_t ws_bytes, void *stream) {
    if (!Q) return fail(SD_ERR_INVALID, "null pointer");
    return spatial_sums_of(X, T, n, st, sn, select_columns(Q), m, out, field, ws, ws_bytes, stream);
}

// ---- K22 ----
static bool lens_sized(i64 T, i64 n, i64 m) { return T >= 1 && n >= 2 && n <= LN_MAX_N && m >= 0 && T < ((i64)1 << 31); }

size_t sd_lens_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m) {
    return metric_workspace_bytes(lens_sized(T, n, m), T, n, st, sn, m, [&](PlanSize z) { return lens_plan(n, m, z); });
}

size_t sd_lens_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m) {
    return metric_min_workspace_bytes(lens_sized(T, n, m), T, n, st, sn, m, [&](PlanSize z) { return lens_plan(n, m, z); });
}

int64_t sd_lens_targets_per_batch(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t m, size_t ws_bytes) {
    return metric_targets_per_batch(lens_sized(T, n, m), T, n, st, sn, ws_bytes, [&](PlanSize z) { return lens_plan(n, m, z); });
}

// K20's refusals, but in an order of their own that the refusal tests pin: m, kappa and algo behind the shape, the matrix' cap
// behind the two curves; the budget counts the matrix and the targets' rows, n (n + m) T pair-timepoints
static int check_lens(const double *X, i64 T, i64 n, i64 st, i64 sn, CurveSel sel, i64 m, const void *out, double kappa, int algo) {
    if (!X || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (T < 1 || n < 1) return fail(SD_ERR_INVALID, "bad shape (T=%lld, n=%lld): at least one timepoint", (long long)T, (long long)n);
    if (m < 0) return fail(SD_ERR_INVALID, "m < 0");
    if (!(kappa >= -1.0 && kappa <= 1.0)) return fail(SD_ERR_INVALID, "kappa = 2 / beta - 1 must lie in [-1, 1], got %g", kappa);
    if (algo < 0 || algo > 1) return fail(SD_ERR_INVALID, "algo=%d outside {0 (the form by kappa), 1 (the general form)}", algo);
    if (n < 2) return fail(SD_ERR_UNSUPPORTED, "distances between curves need at least two curves, got %lld", (long long)n);
    if (n > LN_MAX_N)
        return fail(SD_ERR_UNSUPPORTED, "the lune depths keep the n x n matrix of distances: at most %lld curves, got %lld",
                    (long long)LN_MAX_N, (long long)n);
    int rc = sel.Q ? check_matrix(X, T, n, st, sn, nullptr, n) : check_matrix(X, T, n, st, sn, sel.targets, m);
    if (rc) return rc;
    const double work = (double)n * ((double)n + (double)m) * (double)T;
    if (work > HS_MAX_WORK) return fail(SD_ERR_UNSUPPORTED, "%.3g pair-timepoints exceed the cap of %.0e", work, HS_MAX_WORK);
    return SD_OK;
}

static int lens_counts_of(const double *X, i64 T, i64 n, i64 st, i64 sn, CurveSel sel, i64 m, double kappa, int algo, i64 *out, void *ws,
                          size_t ws_bytes, void *stream) {
    int rc = check_lens(X, T, n, st, sn, sel, m, out, kappa, algo);
    if (rc || m == 0) return rc;
    return launch_time_major(X, T, n, st, sn, ws, ws_bytes, sd_lens_min_workspace_bytes(T, n, st, sn, m), "sd_lens_min_workspace_bytes",
                             stream, [&](const double *Y, void *w, size_t bytes, hipStream_t s) {
                                 return launch_lens_counts(Y, T, n, sel, m, kappa, algo, out, w, bytes, s);
                             });
}

int sd_lens_counts(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const int64_t *targets, int64_t m, double kappa,
                   int algo, int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    return lens_counts_of(X, T, n, st, sn, select_sample(targets), m, kappa, algo, out, ws, ws_bytes, stream);
}

int sd_lens_external_counts(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *Q, int64_t m, double kappa,
                            int algo, int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    if (!Q) return fail(SD_ERR_INVALID, "null pointer");
    return lens_counts_of(X, T, n, st, sn, select_columns(Q), m, kappa, algo, out, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------
// K18
// ---------------------------------------------------------------------------
int64_t sd_multi_cloud_lds_capacity(void) { return MC_LDS_CAPACITY; }

// the route of a call the size functions answer for (0: none)
static int multi_cloud_sized_route(i64 n, i64 T, int d, i64 k, i64 m, int algo) {
    if (n < 1 || T < 1 || d < 1 || d > 8 || k < 1 || m < 0 || n >= ((i64)1 << 31) || algo < 0 || algo > 2) return 0;
    return multi_cloud_route(algo, n);
}

// K10's / K12's checks in their order and wording, with T clouds of n points; then algo, the targets, the route and the
// floor of the workspace (extra: the batch consumer's own bytes per timepoint; family: the name in the size functions)
static int multi_cloud_checked(bool proj, const double *P, i64 n, i64 T, int d, const double *U, i64 k, const i64 *targets, i64 m,
                               int algo, void *out, void *ws, size_t ws_bytes, size_t extra, const char *family, int &route) {
    const double work = (double)T * (double)k * (double)n * ((double)d + log2_steps(n));
    if (!P || !U || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (T < 1) return fail(SD_ERR_INVALID, "bad shape (T=%lld): at least one timepoint", (long long)T);
    int rc = proj ? check_projection(P, n, d, U, k, m, out, n, work) : check_halfspace(P, n, d, U, k, m, out, n, work);
    if (rc) return rc;
    if (algo < 0 || algo > 2) return fail(SD_ERR_INVALID, "algo=%d outside 0 (auto), 1 (lds), 2 (global)", algo);
    if (!targets && m != n) return fail(SD_ERR_INVALID, "targets=NULL requires m == n");
    route = multi_cloud_route(algo, n);
    if (route == 0)
        return fail(SD_ERR_UNSUPPORTED, "the LDS route holds clouds of up to %lld curves, got %lld (algo 0 or 2 takes them)",
                    (long long)MC_LDS_CAPACITY, (long long)n);
    if (!ws || ws_bytes < multi_cloud_min_workspace_bytes(route, proj, n, d, extra))
        return fail(SD_ERR_WORKSPACE, "workspace too small for one timepoint per batch (sd_multi_%s_min_workspace_bytes)", family);
    return SD_OK;
}

static int multi_cloud_sums(bool proj, const double *P, i64 n, i64 T, int d, const double *U, i64 k, const i64 *targets, i64 m,
                            int algo, void *out, void *ws, size_t ws_bytes, void *stream) {
    int route;
    int rc = multi_cloud_checked(proj, P, n, T, d, U, k, targets, m, algo, out, ws, ws_bytes, 0,
                                 proj ? "projection" : "halfspace", route);
    if (rc || m == 0) return rc;
    return launch_multi_cloud(proj, route, P, n, T, d, U, k, targets, m, out, ws, ws_bytes, (hipStream_t)stream);
}

size_t sd_multi_halfspace_workspace_bytes(int64_t n, int64_t T, int d, int64_t k, int64_t m, int algo) {
    const int route = multi_cloud_sized_route(n, T, d, k, m, algo);
    return route ? multi_cloud_workspace_bytes(route, false, n, T, d, k) : 0;
}

size_t sd_multi_halfspace_min_workspace_bytes(int64_t n, int64_t T, int d, int64_t k, int64_t m, int algo) {
    const int route = multi_cloud_sized_route(n, T, d, k, m, algo);
    return route ? multi_cloud_min_workspace_bytes(route, false, n, d) : 0;
}

int sd_multi_halfspace_sums(const double *P, int64_t n, int64_t T, int d, const double *U, int64_t k, const int64_t *targets,
                            int64_t m, int algo, int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    return multi_cloud_sums(false, P, n, T, d, U, k, targets, m, algo, out, ws, ws_bytes, stream);
}

size_t sd_multi_projection_workspace_bytes(int64_t n, int64_t T, int d, int64_t k, int64_t m, int algo) {
    const int route = multi_cloud_sized_route(n, T, d, k, m, algo);
    return route ? multi_cloud_workspace_bytes(route, true, n, T, d, k) : 0;
}

size_t sd_multi_projection_min_workspace_bytes(int64_t n, int64_t T, int d, int64_t k, int64_t m, int algo) {
    const int route = multi_cloud_sized_route(n, T, d, k, m, algo);
    return route ? multi_cloud_min_workspace_bytes(route, true, n, d) : 0;
}

int sd_multi_projection_sums(const double *P, int64_t n, int64_t T, int d, const double *U, int64_t k, const int64_t *targets,
                             int64_t m, int algo, double *out, void *ws, size_t ws_bytes, void *stream) {
    return multi_cloud_sums(true, P, n, T, d, U, k, targets, m, algo, out, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------
// K19
// ---------------------------------------------------------------------------
size_t sd_multi_outlyingness_workspace_bytes(int64_t n, int64_t T, int d, int64_t k, int64_t m, int algo) {
    const int route = multi_cloud_sized_route(n, T, d, k, m, algo);
    return route ? multi_cloud_workspace_bytes(route, true, n, T, d, k, DO_EXTRA) : 0;
}

size_t sd_multi_outlyingness_min_workspace_bytes(int64_t n, int64_t T, int d, int64_t k, int64_t m, int algo) {
    const int route = multi_cloud_sized_route(n, T, d, k, m, algo);
    return route ? multi_cloud_min_workspace_bytes(route, true, n, d, DO_EXTRA) : 0;
}

int sd_multi_outlyingness_moments(const double *P, int64_t n, int64_t T, int d, const double *U, int64_t k,
                                  const int64_t *targets, int64_t m, int algo, double *out, int64_t *centres, double *curves,
                                  void *ws, size_t ws_bytes, void *stream) {
    int route;
    int rc = multi_cloud_checked(true, P, n, T, d, U, k, targets, m, algo, out, ws, ws_bytes, DO_EXTRA, "outlyingness", route);
    if (rc || m == 0) return rc;
    return launch_multi_outlyingness(route, P, n, T, d, U, k, targets, m, out, centres, curves, ws, ws_bytes, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// K23: the projections of curves (include/statdepth_hip_projections.h, curve_project.hip)
// ---------------------------------------------------------------------------
// The refusals the three entry points share, in their order; n_min: the fewest curves (1 for the projections alone).
// comparisons: per projected value, what the call does with Z (0 for the projections alone).
static int check_curve_projections(const double *X, i64 T, i64 n, i64 st, i64 sn, const double *U, i64 k, const i64 *targets,
                                   i64 m, const void *out, i64 n_min, int algo, double comparisons) {
    if (!X || !U || !out) return fail(SD_ERR_INVALID, "null pointer");
    if (T < 1 || k < 1 || n < n_min)
        return fail(SD_ERR_INVALID, "bad shape (T=%lld, n=%lld, k=%lld): at least one timepoint, one direction and %lld curve(s)",
                    (long long)T, (long long)n, (long long)k, (long long)n_min);
    int rc;
    if ((rc = refuse_algo(algo, RD_ALGO_NAMES)) || (rc = refuse_curves(n, "the projections of curves take"))) return rc;
    if (T >= ((i64)1 << 31) || k >= ((i64)1 << 31))
        return fail(SD_ERR_UNSUPPORTED, "the projections of curves take fewer than 2^31 timepoints and directions");
    if ((rc = refuse_route1(algo, n, "image"))) return rc;
    const double work = (double)k * (double)n * ((double)T + comparisons);
    if (work > HS_MAX_WORK)
        return fail(SD_ERR_UNSUPPORTED, "%.3g multiply-adds and comparisons exceed the cap of %.0e", work, HS_MAX_WORK);
    return check_matrix(X, T, n, st, sn, targets, m);
}

static bool rp_shape(i64 T, i64 n, i64 k, i64 n_min) {
    const i64 lim = (i64)1 << 31;
    return T >= 1 && k >= 1 && n >= n_min && T < lim && n < lim && k < lim;
}

size_t sd_curve_projections_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t k) {
    (void)T, (void)n, (void)st, (void)sn, (void)k;
    return 0;
}

int sd_curve_projections(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *U, int64_t k, double *out,
                         void *ws, size_t ws_bytes, void *stream) {
    (void)ws, (void)ws_bytes;
    const int rc = check_curve_projections(X, T, n, st, sn, U, k, nullptr, n, out, 1, 0, 0.0);
    return rc ? rc : launch_curve_project(X, T, n, st, sn, U, 0, k, out, (hipStream_t)stream);
}

size_t sd_rp_depth_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t k, int64_t m, int algo) {
    (void)st, (void)sn, (void)m;
    const int route = rp_shape(T, n, k, 2) ? curve_route(algo, k, n) : 0;
    return route ? rp_depth_plan(n, k, route, PlanSize::of_rows(k)).bytes : 0;
}

size_t sd_rp_depth_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t k, int64_t m, int algo) {
    (void)st, (void)sn, (void)m;
    const int route = rp_shape(T, n, k, 2) ? curve_route(algo, k, n) : 0;
    return route ? rp_depth_plan(n, k, route, PlanSize::of_rows(1)).bytes : 0;
}

int sd_rp_depth_sums(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *U, int64_t k,
                     const int64_t *targets, int64_t m, int algo, int64_t *out, void *ws, size_t ws_bytes, void *stream) {
    const int rc = check_curve_projections(X, T, n, st, sn, U, k, targets, m, out, 2, algo, log2_steps(n));
    if (rc || m == 0) return rc;
    if (!ws || ws_bytes < sd_rp_depth_min_workspace_bytes(T, n, st, sn, k, m, algo))
        return fail(SD_ERR_WORKSPACE, "workspace below sd_rp_depth_min_workspace_bytes");
    return launch_rp_depth_sums(X, T, n, st, sn, U, k, targets, m, curve_route(algo, k, n), out, ws, ws_bytes, (hipStream_t)stream);
}

size_t sd_rp_outlyingness_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t k, int64_t m) {
    (void)st, (void)sn, (void)m;
    return rp_shape(T, n, k, 2) ? rp_outlyingness_workspace_bytes(n, k) : 0;
}

size_t sd_rp_outlyingness_min_workspace_bytes(int64_t T, int64_t n, int64_t st, int64_t sn, int64_t k, int64_t m) {
    (void)st, (void)sn, (void)m;
    return rp_shape(T, n, k, 2) ? rp_outlyingness_min_workspace_bytes(n) : 0;
}

int sd_rp_outlyingness(const double *X, int64_t T, int64_t n, int64_t st, int64_t sn, const double *U, int64_t k,
                       const int64_t *targets, int64_t m, double *out, void *ws, size_t ws_bytes, void *stream) {
    const int rc = check_curve_projections(X, T, n, st, sn, U, k, targets, m, out, 2, 0, log2_steps(n));
    if (rc || m == 0) return rc;
    return launch_rp_outlyingness(X, T, n, st, sn, U, k, targets, m, out, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
