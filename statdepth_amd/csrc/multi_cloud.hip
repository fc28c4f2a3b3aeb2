// multi_cloud.hip -- K18: halfspace and projection depth of multivariate curves, integrated over time.
//
// Definition.  n curves, T timepoints, d <= 8 features, P[i][t][e] row-major; directions u_0 .. u_(k-1) (k x d) shared by
// all timepoints.  The cloud at t is C_t = {P[i][t][:]}, n points, the target among them.
//   h_t(i) = K10's count of point i in C_t: min over r of min(ge_r, le_r), the point and every tie counted (halfspace.hip);
//   O_t(i) = K12's outlyingness of point i in C_t: max over r of |z_r - med_r| / mad_r (projection.hip);
// both on K10's projection bits (hs_proj).  Per target:
//   halfspace:   SH = sum_t h_t (int64),  MH = min_t h_t;
//   projection:  PS = sum_t 1 / (1 + O_t), each term one rounded addition and one correctly rounded division (O = inf:
//                0.0), added in ascending t from 0.0 with one rounded addition per timepoint (np.cumsum's order);
//                OM = max_t O_t.
// Integer min and sum and the maximum of non-negative doubles are order-free; PS is added by one owner per target in
// ascending t in every configuration, its partial sum carried in out[] across the batches in stream order.  So nothing
// depends on the route, the workspace size or how directions and timepoints are split.
//
// The timepoints are taken in batches of Tb (what the workspace holds).  Per batch both routes leave V[tb][i], the value
// of EVERY curve i at timepoint t0 + tb, in the workspace, and hand the batch to a consumer (McBatch, McConsumer) once every
// slice of it has been launched.  K18's consumer is mc_fold_kernel (a thread per target), which adds the batch's timepoints
// to out[] in ascending t; K19's (directional_out.hip) takes the centre of each cloud and folds the directional
// outlyingness.  There is one batch loop per route, whoever consumes.
//
// LDS route (n <= MC_LDS_CAPACITY = 8192):
//   the batch is copied feature-major, Y[tb][e][i] (launch_to_time_major, a tiled transpose): the input's point stride is
//   T d doubles, so a cloud gathered from P touches one cache line per point and uses d / 8 of it, once per direction
//   slice; from Y a wave reads 512 contiguous bytes per feature;
//   mc_lds_kernel, one workgroup of 1024 threads per (timepoint, slice of MC_SLICE = 32 directions): per direction every
//   thread projects its points (at most 8, point i = thread + 1024 j; their projections stay in registers), the
//   workgroup sorts the keys alone in LDS (the bitonic network of the next power of two, the pairs past n left out), and every
//   thread places its own projections in the sorted keys: halfspace by a lower and an upper bound (lt and le, ties
//   counted), projection through K12's selection (pd_locscale on the LDS array, evaluated by every thread at the same
//   addresses: LDS broadcasts, no barrier, nothing shared).  The running minimum count or maximum outlyingness of a
//   thread's points stays in registers across the slice; slices of one timepoint meet in V through atomicMin on u32 /
//   atomicMax on the 64-bit pattern (non-negative doubles order like their patterns): exact and order-free.
//   No index travels through the sort: 8 bytes per key, 64 KB of LDS per workgroup.
// Global route (any n K10 / K12 take): per timepoint mc_gather_kernel copies the cloud to a dense n x d array and K10's
//   or K12's own chunked launcher (project, tile sort, merge passes, rank or locscale + outlyingness) writes V for
//   Tb = 1.  The cross-check of the LDS route and the route above its capacity.
//
// Every launch is bounded: an mc_lds_kernel launch has at most MC_UNITS = 512 workgroups of at most 32 sorts of at most
// 8192 keys; the global route's launches are K10's and K12's.  No kernel waits on another workgroup.
#include <type_traits>
#include "sd_common.h"
#include "multi_cloud_batches.h"
#include "point_select.h"
#include "projection_select.h"

namespace sd {

constexpr int MC_THREADS = 1024;
constexpr int MC_PPT = (int)(MC_LDS_CAPACITY / MC_THREADS);        // points per thread
constexpr int MC_SLICE = 32;                                       // directions per workgroup
constexpr u64 MC_UNITS = 512;                                      // workgroups per launch
constexpr int MC_FOLD_THREADS = 256;
constexpr i64 MC_REC_VALUES = (i64)1 << 25;                        // coordinates per batch of the recommended workspace
constexpr i64 MC_MAX_BATCH = (i64)1 << 17;                         // timepoints per batch (the transpose's grid: Tb d / 32 rows)
static_assert(MC_PPT * MC_THREADS == MC_LDS_CAPACITY && (MC_LDS_CAPACITY & (MC_LDS_CAPACITY - 1)) == 0,
              "the bitonic network pads a cloud to a power of two inside sk[]");

// ---------------------------------------------------------------------------------------------- LDS route
// unit u0 + blockIdx.x = tb * S + slice;  Y: the batch feature-major, Y[tb][e][i];  V[tb][i]: u32 counts (0xffffffff
// before the first slice) or the 64-bit patterns of the outlyingness (0 before)
template <int D, bool PROJ>
__global__ __launch_bounds__(MC_THREADS) void mc_lds_kernel(const double *__restrict__ Y, int n,
                                                            const double *__restrict__ U, i64 k, u64 S, u64 u0,
                                                            void *__restrict__ V) {
    __shared__ double sk[MC_LDS_CAPACITY];
    const u64 unit = u0 + blockIdx.x;
    const i64 tb = (i64)(unit / S);
    const i64 r0 = (i64)(unit % S) * MC_SLICE;
    const i64 r1 = r0 + MC_SLICE < k ? r0 + MC_SLICE : k;
    const double *Yt = Y + tb * D * (i64)n;
    int N2 = 1;
    while (N2 < n) N2 <<= 1;
    u32 cbest[MC_PPT];
    double obest[MC_PPT];
#pragma unroll
    for (int j = 0; j < MC_PPT; ++j) {
        cbest[j] = 0xffffffffu;
        obest[j] = 0.0;
    }
    for (i64 r = r0; r < r1; ++r) {
        // hs_proj's operations in its order, a feature at a time over the thread's points (one feature row of Y in flight,
        // not D of them: no spills at d = 8)
        double z[MC_PPT];
        const double uf = U[r * D];                                 // wave-uniform
#pragma unroll
        for (int j = 0; j < MC_PPT; ++j) {
            const int i = threadIdx.x + j * MC_THREADS;
            z[j] = i < n ? __dmul_rn(Yt[i], uf) : 0.0;
        }
#pragma unroll 1
        for (int e = 1; e < D; ++e) {
            const double ue = U[r * D + e];
            const double *Ye = Yt + (i64)e * n;
#pragma unroll
            for (int j = 0; j < MC_PPT; ++j) {
                const int i = threadIdx.x + j * MC_THREADS;
                if (i < n) z[j] = __dadd_rn(z[j], __dmul_rn(Ye[i], ue));
            }
        }
#pragma unroll
        for (int j = 0; j < MC_PPT; ++j) {
            const int i = threadIdx.x + j * MC_THREADS;
            if (i < n) sk[i] = z[j];
        }
        __syncthreads();
        // The bitonic network of N2 slots in its all-ascending form: per level kk the first stage pairs a slot with its
        // mirror image inside the block of kk (i ^ (kk - 1)), the others with i | jj; every exchange leaves the smaller key
        // at the lower slot.  Slots n .. N2 - 1 are virtual +inf: an exchange with one of them would change nothing, so the
        // pairs that reach past n are left out and the padding is neither stored nor moved.
        for (int kk = 2; kk <= N2; kk <<= 1) {
            for (int jj = kk >> 1; jj > 0; jj >>= 1) {
                const bool mirror = jj == (kk >> 1);
                for (int x = threadIdx.x; x < (N2 >> 1); x += MC_THREADS) {
                    const int i = ((x & ~(jj - 1)) << 1) | (x & (jj - 1));
                    const int l = mirror ? i ^ (kk - 1) : i | jj;
                    if (l < n) {
                        const double a = sk[i], b = sk[l];
                        if (a > b) {
                            sk[i] = b;
                            sk[l] = a;
                        }
                    }
                }
                __syncthreads();
            }
        }
        // sk[0 .. n) holds the cloud's projections ascending
        if constexpr (PROJ) {
            double med, mad;
            pd_locscale(PdLdsRow{sk}, n, med, mad);                 // every thread, the same addresses: broadcast reads
#pragma unroll
            for (int j = 0; j < MC_PPT; ++j) {
                if ((int)threadIdx.x + j * MC_THREADS < n) {
                    const double o = pd_outlyingness(z[j], med, mad);
                    obest[j] = o > obest[j] ? o : obest[j];
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < MC_PPT; ++j) {
                if ((int)threadIdx.x + j * MC_THREADS < n) {
                    const double key = z[j];
                    int lo = 0, hi = n;
                    while (lo < hi) {                               // lt = #{keys < key}
                        const int mid = (lo + hi) >> 1;
                        if (sk[mid] < key) lo = mid + 1;
                        else hi = mid;
                    }
                    const int lt = lo;
                    hi = n;
                    while (lo < hi) {                               // le = #{keys <= key}, at or behind lt
                        const int mid = (lo + hi) >> 1;
                        if (sk[mid] <= key) lo = mid + 1;
                        else hi = mid;
                    }
                    const int le = lo, ge = n - lt;
                    const u32 c = (u32)(le < ge ? le : ge);
                    cbest[j] = c < cbest[j] ? c : cbest[j];
                }
            }
        }
        __syncthreads();                                            // the keys have been read before the next projection
    }
#pragma unroll
    for (int j = 0; j < MC_PPT; ++j) {
        const int i = threadIdx.x + j * MC_THREADS;
        if (i < n) {
            if constexpr (PROJ) {
                if (obest[j] > 0.0) atomicMax((u64 *)V + tb * n + i, (u64)__double_as_longlong(obest[j]));
            } else {
                atomicMin((u32 *)V + tb * n + i, cbest[j]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- global route
// C[i][e] = P[i][t][e]: the cloud at t as the dense n x d array K10 and K12 take
__global__ __launch_bounds__(MC_FOLD_THREADS) void mc_gather_kernel(const double *__restrict__ P, i64 n, i64 T, int d, i64 t,
                                                                    double *__restrict__ C) {
    const i64 g = (i64)blockIdx.x * MC_FOLD_THREADS + threadIdx.x;
    if (g >= n * d) return;
    const i64 i = g / d;
    const int e = (int)(g % d);
    C[g] = P[(i * T + t) * d + e];
}

// ---------------------------------------------------------------------------------------------- fold
// a thread per target: the batch's Tb timepoints added to out[q] (m x 2) in ascending t; first: the batch starts the record.
// halfspace (V = u32 or int64 counts): SH += v, MH = min(MH, v);  projection (V = double): PS += 1 / (1 + o), OM = max
template <class V>
__global__ __launch_bounds__(MC_FOLD_THREADS) void mc_fold_kernel(const V *__restrict__ W, i64 n, i64 Tb,
                                                                  const i64 *__restrict__ targets, i64 m, int first,
                                                                  void *__restrict__ out) {
    const i64 q = (i64)blockIdx.x * MC_FOLD_THREADS + threadIdx.x;
    if (q >= m) return;
    const i64 row = targets ? targets[q] : q;
    if constexpr (std::is_floating_point<V>::value) {
        double *o = (double *)out + 2 * q;
        double ps = first ? 0.0 : o[0], om = first ? 0.0 : o[1];
        for (i64 t = 0; t < Tb; ++t) {
            const double v = W[t * n + row];
            ps = __dadd_rn(ps, __ddiv_rn(1.0, __dadd_rn(1.0, v)));
            om = v > om ? v : om;
        }
        o[0] = ps;
        o[1] = om;
    } else {
        i64 *o = (i64 *)out + 2 * q;
        i64 sh = first ? 0 : o[0], mh = first ? INT64_MAX : o[1];
        for (i64 t = 0; t < Tb; ++t) {
            const i64 v = (i64)W[t * n + row];
            sh += v;
            mh = v < mh ? v : mh;
        }
        o[0] = sh;
        o[1] = mh;
    }
}

template <class V>
static int launch_mc_fold(const V *W, i64 n, i64 Tb, const i64 *targets, i64 m, int first, void *out, hipStream_t s) {
    hipLaunchKernelGGL((mc_fold_kernel<V>), dim3((unsigned)((m + MC_FOLD_THREADS - 1) / MC_FOLD_THREADS)),
                       dim3(MC_FOLD_THREADS), 0, s, W, n, Tb, targets, m, first, out);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------- plan and launchers
int multi_cloud_route(int algo, i64 n) {
    if (algo == 2) return 2;
    if (n <= MC_LDS_CAPACITY) return 1;
    return algo == 0 ? 2 : 0;
}

// LDS route: Y (8 n d bytes per timepoint), V (4 or 8 n) and the consumer's extra bytes, each padded to 256 bytes
static inline size_t mc_lds_per_timepoint(bool proj, i64 n, int d, size_t extra) {
    return (size_t)n * ((size_t)d * 8 + (proj ? 8 : 4)) + extra;
}
static inline size_t mc_lds_fixed(size_t extra) { return (extra ? 3 : 2) * 256; }
// global route: the cloud (8 n d), V (8 n) and the extra bytes, each padded to 256 bytes, in front of K10's or K12's own workspace
static inline size_t mc_global_fixed(i64 n, int d, size_t extra) {
    return align_up((size_t)n * d * 8, 256) + align_up((size_t)n * 8, 256) + align_up(extra, 256) + 256;
}

size_t multi_cloud_min_workspace_bytes(int route, bool proj, i64 n, int d, size_t extra) {
    if (route == 1) return mc_lds_fixed(extra) + mc_lds_per_timepoint(proj, n, d, extra);
    return mc_global_fixed(n, d, extra) + (proj ? projection_min_workspace_bytes(n) : halfspace_min_workspace_bytes(n));
}

size_t multi_cloud_workspace_bytes(int route, bool proj, i64 n, i64 T, int d, i64 k, size_t extra) {
    if (route == 1) {
        i64 Tb = MC_REC_VALUES / (n * d);
        Tb = Tb < 1 ? 1 : Tb > T ? T : Tb;
        return mc_lds_fixed(extra) + (size_t)Tb * mc_lds_per_timepoint(proj, n, d, extra);
    }
    return mc_global_fixed(n, d, extra) + (proj ? projection_workspace_bytes(n, k) : halfspace_workspace_bytes(n, k));
}

template <int D, bool PROJ>
static int launch_mc_lds_d(const double *P, i64 n, i64 T, const double *U, i64 k, size_t extra, const McConsumer &consume,
                           void *ws, size_t ws_bytes, hipStream_t s) {
    const size_t per = mc_lds_per_timepoint(PROJ, n, D, extra);
    i64 Tb = (i64)((ws_bytes - mc_lds_fixed(extra)) / per);         // (the caller has checked the floor)
    Tb = Tb > T ? T : Tb > MC_MAX_BATCH ? MC_MAX_BATCH : Tb;
    const size_t vbytes = PROJ ? 8 : 4;
    Carver cv(ws, ws_bytes);
    double *Y = (double *)cv.take((size_t)Tb * n * D * 8);
    void *V = cv.take((size_t)Tb * n * vbytes);
    void *X = extra ? cv.take((size_t)Tb * extra) : nullptr;
    if (Tb < 1 || !Y || !V || (extra && !X)) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_multi_*_min_workspace_bytes)");
    const u64 S = (u64)((k + MC_SLICE - 1) / MC_SLICE);
    for (i64 t0 = 0; t0 < T; t0 += Tb) {
        const i64 tb = T - t0 < Tb ? T - t0 : Tb;
        // rows (tb', e) of Y from the unit-stride runs of P: Y[(tb' D + e) n + i] = P[i T D + (t0 + tb') D + e]
        int rc = launch_to_time_major(P + t0 * D, tb * D, n, 1, T * D, Y, s);
        if (rc) return rc;
        SD_HIP(hipMemsetAsync(V, PROJ ? 0 : 0xff, (size_t)tb * n * vbytes, s));
        const u64 units = (u64)tb * S;
        for (u64 u0 = 0; u0 < units; u0 += MC_UNITS) {
            const u64 g = units - u0 < MC_UNITS ? units - u0 : MC_UNITS;
            hipLaunchKernelGGL((mc_lds_kernel<D, PROJ>), dim3((unsigned)g), dim3(MC_THREADS), 0, s, Y, (int)n, U, k, S, u0, V);
            SD_HIP(hipGetLastError());
        }
        if ((rc = consume(McBatch{V, Y, true, X, t0, tb}, s))) return rc;   // V is final: every slice has met in it
    }
    return SD_OK;
}

static int launch_mc_global(bool proj, const double *P, i64 n, i64 T, int d, const double *U, i64 k, size_t extra,
                            const McConsumer &consume, void *ws, size_t ws_bytes, hipStream_t s) {
    Carver cv(ws, ws_bytes);
    double *C = (double *)cv.take((size_t)n * d * 8);
    void *V = cv.take((size_t)n * 8);
    void *X = extra ? cv.take(extra) : nullptr;
    const size_t inner_bytes = cv.rest();
    void *inner = cv.take(inner_bytes);
    if (!C || !V || !inner || (extra && !X)) return fail(SD_ERR_WORKSPACE, "workspace too small (sd_multi_*_min_workspace_bytes)");
    for (i64 t = 0; t < T; ++t) {
        hipLaunchKernelGGL(mc_gather_kernel, dim3((unsigned)((n * d + MC_FOLD_THREADS - 1) / MC_FOLD_THREADS)),
                           dim3(MC_FOLD_THREADS), 0, s, P, n, T, d, t, C);
        SD_HIP(hipGetLastError());
        int rc;
        if (proj) rc = launch_projection_sorted(C, n, d, U, k, select_rows(nullptr), n, (double *)V, inner, inner_bytes, s);
        else rc = launch_halfspace_counts(C, n, d, U, k, nullptr, n, (i64 *)V, inner, inner_bytes, s);
        if (!rc) rc = consume(McBatch{V, C, false, X, t, 1}, s);
        if (rc) return rc;
    }
    return SD_OK;
}

int launch_multi_cloud_batches(bool proj, int route, const double *P, i64 n, i64 T, int d, const double *U, i64 k, size_t extra,
                               const McConsumer &consume, void *ws, size_t ws_bytes, hipStream_t s) {
    if (!ws || ws_bytes < multi_cloud_min_workspace_bytes(route, proj, n, d, extra))
        return fail(SD_ERR_WORKSPACE, "workspace too small for one timepoint per batch (sd_multi_*_min_workspace_bytes)");
    if (route == 2) return launch_mc_global(proj, P, n, T, d, U, k, extra, consume, ws, ws_bytes, s);
    if (proj) {
        SD_DISPATCH_D(d, return (launch_mc_lds_d<D_, true>(P, n, T, U, k, extra, consume, ws, ws_bytes, s)))
    } else {
        SD_DISPATCH_D(d, return (launch_mc_lds_d<D_, false>(P, n, T, U, k, extra, consume, ws, ws_bytes, s)))
    }
    return fail(SD_ERR_UNSUPPORTED, "multivariate curve depths cover d in [1,8], got %d", d);
}

// K18's own consumer: the fold of the batch into the records (SH, MH) / (PS, OM)
int launch_multi_cloud(bool proj, int route, const double *P, i64 n, i64 T, int d, const double *U, i64 k, const i64 *targets,
                       i64 m, void *out, void *ws, size_t ws_bytes, hipStream_t s) {
    return launch_multi_cloud_batches(proj, route, P, n, T, d, U, k, 0, [=](const McBatch &b, hipStream_t st) {
        if (proj) return launch_mc_fold((const double *)b.V, n, b.tb, targets, m, b.t0 == 0, out, st);
        if (b.feature_major) return launch_mc_fold((const u32 *)b.V, n, b.tb, targets, m, b.t0 == 0, out, st);
        return launch_mc_fold((const i64 *)b.V, n, b.tb, targets, m, b.t0 == 0, out, st);
    }, ws, ws_bytes, s);
}

}  // namespace sd
