// directional_out.hip -- K19: directional outlyingness of multivariate curves (Dai & Genton), the records of the MS-plot.
//
// Definition.  P, U as in K18 (multi_cloud.hip).  Per timepoint t:
//   o_t(i) = K18's O_t(i), the Stahel-Donoho outlyingness of point i inside the cloud at t (what both routes leave in V);
//   c_t    = the LOWEST curve index among those minimising o_t over ALL n curves: the sample point of largest projection
//            depth, the cloud's median over the direction set;
//   diff_e = P[i][t][e] - P[c_t][t][e];  s = sum_e diff_e^2 in ascending e (one rounded multiplication and one rounded
//            addition per term);  r = sqrt(s), correctly rounded;
//   O_t(i)_e = o_t(i) * (diff_e / r): one rounded division, one rounded multiplication;  r == 0: the zero vector (the centre,
//            its duplicates, differences whose squares underflow).  o = +inf is not special-cased: +-inf, NaN where diff_e = 0.
// Per target, over ascending t, a Welford record of d running means M_e and one running sum Q, from 0.0: with
// c = (double)(t + 1), for e ascending
//   delta = O_e - M_e;  M_e = M_e + delta / c;  Q = Q + delta * (O_e - M_e)          (every operation rounded once)
// out[q] = (M_0 .. M_(d-1), Q).  Host: MO = M, VO = Q / T, FO = |MO|^2 + VO.
//
// Nothing depends on the route, the workspace size or how directions and timepoints are split: o_t is order-free (K18), c_t
// is an argmin with a fixed tie rule, and the record has one owner per target in ascending t, carried in out[] across the
// batches in stream order.
//
// The expensive stage (project, sort, select) is K18's, through its batch loop (launch_multi_cloud_batches); this file is
// the loop's consumer: two kernels per batch on what the workspace already holds.
//   do_centre_kernel   one workgroup per timepoint of the batch: the lexicographic minimum of (pattern of o, index) over the
//                      n curves (non-negative doubles order like their patterns, +inf last) -> Cn[tb], and centres[t0 + tb];
//   do_moments_kernel  a thread per target walks the batch in ascending t: the point and the centre from the feature-major
//                      copy Y[tb][e][.] (lds route: coalesced across targets, the centre a broadcast) or from the gathered
//                      cloud C (global route, tb = 1); M in registers (template on D).
// Every launch is bounded (at most MC_MAX_BATCH workgroups of n loads; m threads of tb timepoints); no kernel waits on another
// workgroup.
#include "multi_cloud_batches.h"

namespace sd {

constexpr int DO_CENTRE_THREADS = 1024;
constexpr int DO_FOLD_THREADS = 64;                                // a wave per workgroup: the targets spread over the CUs

// (pattern, index) below (pattern', index')
__device__ __forceinline__ bool do_less(u64 p, i64 i, u64 q, i64 j) { return p < q || (p == q && i < j); }

__global__ __launch_bounds__(DO_CENTRE_THREADS) void do_centre_kernel(const double *__restrict__ V, i64 n, i64 t0,
                                                                       i64 *__restrict__ Cn, i64 *__restrict__ centres) {
    __shared__ u64 sp[DO_CENTRE_THREADS / 64];
    __shared__ i64 si[DO_CENTRE_THREADS / 64];
    const i64 tb = blockIdx.x;
    const u64 *W = (const u64 *)V + tb * n;
    u64 bp = ~(u64)0;
    i64 bi = n;                                                     // no curve: above every (pattern, index)
    for (i64 i = threadIdx.x; i < n; i += DO_CENTRE_THREADS) {
        const u64 p = W[i] & 0x7fffffffffffffffull;                 // (o >= 0; a zero keeps one pattern whatever its sign)
        if (p < bp) {                                               // ascending i: the first minimum of the thread stays
            bp = p;
            bi = i;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 qp = (u64)__shfl_down((unsigned long long)bp, off, 64);
        const i64 qi = (i64)__shfl_down((long long)bi, off, 64);
        if (do_less(qp, qi, bp, bi)) {
            bp = qp;
            bi = qi;
        }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sp[wave] = bp;
        si[wave] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < DO_CENTRE_THREADS / 64; ++w) {
            if (do_less(sp[w], si[w], bp, bi)) {
                bp = sp[w];
                bi = si[w];
            }
        }
        Cn[tb] = bi;
        if (centres) centres[t0 + tb] = bi;
    }
}

// FM: pts = Y[tb][e][i];  else pts = C[i][e] and Tb = 1.  out: m x (D + 1);  curves: m x T x D or null
template <int D, bool FM>
__global__ __launch_bounds__(DO_FOLD_THREADS) void do_moments_kernel(const double *__restrict__ V,
                                                                     const double *__restrict__ pts,
                                                                     const i64 *__restrict__ Cn, i64 n, i64 T, i64 t0, i64 Tb,
                                                                     const i64 *__restrict__ targets, i64 m, int first,
                                                                     double *__restrict__ out, double *__restrict__ curves) {
    const i64 q = (i64)blockIdx.x * DO_FOLD_THREADS + threadIdx.x;
    if (q >= m) return;
    const i64 row = targets ? targets[q] : q;
    double *rec = out + q * (D + 1);
    double M[D], Q = first ? 0.0 : rec[D];
#pragma unroll
    for (int e = 0; e < D; ++e) M[e] = first ? 0.0 : rec[e];
    for (i64 t = 0; t < Tb; ++t) {
        const i64 c = Cn[t];                                        // wave-uniform
        const double o = V[t * n + row];
        double diff[D], s = 0.0;
#pragma unroll
        for (int e = 0; e < D; ++e) {
            const double x = FM ? pts[(t * D + e) * n + row] : pts[row * D + e];
            const double xc = FM ? pts[(t * D + e) * n + c] : pts[c * D + e];
            diff[e] = __dsub_rn(x, xc);
            s = __dadd_rn(s, __dmul_rn(diff[e], diff[e]));
        }
        const double r = __dsqrt_rn(s);
        const double cnt = (double)(t0 + t + 1);
#pragma unroll
        for (int e = 0; e < D; ++e) {
            const double O = r == 0.0 ? 0.0 : __dmul_rn(o, __ddiv_rn(diff[e], r));
            const double delta = __dsub_rn(O, M[e]);
            M[e] = __dadd_rn(M[e], __ddiv_rn(delta, cnt));
            Q = __dadd_rn(Q, __dmul_rn(delta, __dsub_rn(O, M[e])));
            if (curves) curves[(q * T + t0 + t) * D + e] = O;
        }
    }
#pragma unroll
    for (int e = 0; e < D; ++e) rec[e] = M[e];
    rec[D] = Q;
}

template <int D, bool FM>
static int launch_do_moments(const McBatch &b, i64 n, i64 T, const i64 *targets, i64 m, double *out, double *curves,
                             hipStream_t s) {
    hipLaunchKernelGGL((do_moments_kernel<D, FM>), dim3((unsigned)((m + DO_FOLD_THREADS - 1) / DO_FOLD_THREADS)),
                       dim3(DO_FOLD_THREADS), 0, s, (const double *)b.V, b.pts, (const i64 *)b.extra, n, T, b.t0, b.tb, targets,
                       m, b.t0 == 0, out, curves);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

int launch_multi_outlyingness(int route, const double *P, i64 n, i64 T, int d, const double *U, i64 k, const i64 *targets, i64 m,
                              double *out, i64 *centres, double *curves, void *ws, size_t ws_bytes, hipStream_t s) {
    static_assert(DO_EXTRA == sizeof(i64), "Cn holds one int64 per timepoint of the batch");
    return launch_multi_cloud_batches(true, route, P, n, T, d, U, k, DO_EXTRA, [=](const McBatch &b, hipStream_t st) {
        hipLaunchKernelGGL(do_centre_kernel, dim3((unsigned)b.tb), dim3(DO_CENTRE_THREADS), 0, st, (const double *)b.V, n, b.t0,
                           (i64 *)b.extra, centres);
        SD_HIP(hipGetLastError());
        if (b.feature_major) {
            SD_DISPATCH_D(d, return (launch_do_moments<D_, true>(b, n, T, targets, m, out, curves, st)))
        } else {
            SD_DISPATCH_D(d, return (launch_do_moments<D_, false>(b, n, T, targets, m, out, curves, st)))
        }
        return fail(SD_ERR_UNSUPPORTED, "directional outlyingness covers d in [1,8], got %d", d);
    }, ws, ws_bytes, s);
}

}  // namespace sd
