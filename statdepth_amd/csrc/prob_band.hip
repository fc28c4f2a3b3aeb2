// prob_band.hip -- K9: band depth (J = 2) of curves observed with independent Gaussian noise (ProbabilisticDepth).
//
// X_c(t) ~ N(mu[t][c], var[t][c]), all independent; var = 0 is a point mass.  For target i, a pair {j, k} of its others
// and a timepoint t, p = P(min(X_j, X_k) <= X_i <= max(X_j, X_k)).  With s_c = sqrt(var_i + var_c), h_c = (mu_i - mu_c)
// / s_c and D_c = (X_i - X_c) / s_c ~ N(h_c, 1), corr(D_j, D_k) = rho = sigma_i^2 / (s_j s_k), p is the probability that
// D_j and D_k differ in sign:
//   p = Phi(h_j) Phi(-h_k) + Phi(-h_j) Phi(h_k) - (1 / pi) int_0^asin(rho) exp((sin(th) h_j h_k - (h_j^2 + h_k^2) / 2)
//       / cos^2(th)) d th    for rho < 0.925 (Drezner-Wesolowsky; Genz 2004, BVND: 6/12/20-point Gauss-Legendre for
//       rho < 0.3 / 0.75 / 0.925)
//     = Phi(hmax) - Phi(hmin) + C(h_j h_k, (h_j - h_k)^2, 1 - rho^2)   for rho >= 0.925 (Genz's branch near |r| = 1; the
//       two orthants share C, and only one of them carries the Phi difference)
// which is BVND's P(D_j > 0, D_k < 0) + P(D_j < 0, D_k > 0), both orthants with correlation -rho.  Written so, p keeps its
// relative accuracy where it is small (the target outside the band), which the strict product needs -- for |h_j|,
// |h_k| <= 12, where tests/test_prob_pairs_gpu.py holds every branch to 1.31e-12 relative against 40-digit values
// (measured on an MI355X: 3.5e-14 in the Gauss-Legendre branches, 3.3e-13 near rho = 1, 2.5e-16 in the degenerate ones).
// Beyond that only the absolute 5e-15 is promised: the 12-point branch still kept 2e-16 relative up to |h| = 38 at
// rho = 0.5, but the branch near rho = 1 drops every term whose exponent is below -100, so from h_j h_k = 200
// on it returns exactly 0 where h_j = h_k (p < 1e-43) and loses digits where they differ (1.3e-4 relative at h = 20, 21).
// 1 - rho^2 = u_j + g_j^2 u_k with g_c = sigma_i / s_c and u_c = sigma_c^2 / s_c^2: no cancellation as rho -> 1
// (sigma_i >> sigma_j, sigma_k).  Degenerate cases, exact and without 0/0:
//   sigma_i = 0:               p = a_j b_k + b_j a_k + e_j + e_k - e_j e_k, a_c = P(X_c > mu_i), b_c = P(X_c < mu_i),
//                              e_c = P(X_c = mu_i) (indicators for point masses; all variances zero: p is 0 or 1 and
//                              the sums equal FunctionalDepth's integer counts)
//   sigma_j = sigma_k = 0 < sigma_i:  p = Phi(hmax) - Phi(hmin), from the tail that keeps digits
//
//   relax:  out[q] = sum_{pairs} sum_t p          strict:  out[q] = sum_{pairs} prod_t p
//
// Work: a unit is (target q, tile of PB_B x PB_B positions of the target's others); a workgroup stages, per chunk of
// PB_TC timepoints, (h, g, u, Phi(h), Phi(-h)) of the tile's 2 PB_B curves in LDS, and each lane walks its PB_PAIRS pairs
// (one j, PB_PAIRS k's) through t.  Per-pair running sums / products live in LDS, and in a state buffer between launches
// when the timepoints are split.  A product that is exactly 0 skips its remaining timepoints (0 * p = 0: same bits).  At
// the last timepoint a lane adds its pairs in order, the workgroup reduces in a fixed tree (pr_block_sum) and
// pn_fold_kernel adds a target's tiles in tile order.  No atomics: a target's bits depend neither on the other targets nor
// on how the call is cut into launches.
//
// Cost: O(m n^2 T) pair evaluations, each an asin and 6-20 sin + exp (or 20 exp and an erfc near rho = 1); fp64 VALU
// and transcendentals are the hot path.  Rates in DESIGN §3 K9 are measured.
#include "prob_common.h"

namespace sd {

constexpr int PB_THREADS = 256;
constexpr int PB_B = 64;                                            // positions per tile side
constexpr int PB_PAIRS = PB_B * PB_B / PB_THREADS;                  // 16 pairs per lane
constexpr int PB_TC = 4;                                            // timepoints staged per chunk
constexpr u64 PB_TILE = (u64)PB_B * PB_B;
// (pair, timepoint) slots per launch: 2^31, about 0.2 s at the measured 10^10 pair evaluations per second
constexpr u64 PB_LAUNCH_EVALS = (u64)1 << 31;
// units per launch when one unit's timepoints alone exceed the cap (then the timepoints are split across launches)
constexpr u64 PB_MIN_UNITS = 2048;
constexpr double PB_HMAX = 1e10;                                    // |h| beyond this: Phi saturated, kept finite

// Gauss-Legendre on [-1, 1]: the positive nodes and their weights, 6, 12 (K8's pn_owen_t uses the same) and 20 points
__constant__ double PB_GL6_X[3] = {0.23861918608319693, 0.6612093864662645, 0.932469514203152};
__constant__ double PB_GL6_W[3] = {0.46791393457269137, 0.36076157304813894, 0.17132449237916975};
__constant__ double PB_GL12_X[6] = {0.1252334085114689, 0.3678314989981802, 0.5873179542866175,
                                        0.7699026741943047, 0.9041172563704748, 0.9815606342467192};
__constant__ double PB_GL12_W[6] = {0.2491470458134027, 0.23349253653835464, 0.20316742672306565,
                                        0.1600783285433461, 0.10693932599531888, 0.04717533638651202};
__constant__ double PB_GL20_X[10] = {0.07652652113349734, 0.2277858511416451, 0.37370608871541955,
                                         0.5108670019508271, 0.636053680726515, 0.7463319064601508,
                                         0.8391169718222188, 0.9122344282513258, 0.9639719272779138,
                                         0.9931285991850949};
__constant__ double PB_GL20_W[10] = {0.15275338713072578, 0.14917298647260366, 0.14209610931838187,
                                         0.13168863844917653, 0.11819453196151825, 0.10193011981724026,
                                         0.08327674157670467, 0.06267204833410944, 0.04060142980038622,
                                         0.017614007139153273};

struct PbCurve {
    double h, g, u, P, Q;                                           // h_c, sigma_i / s_c, sigma_c^2 / s_c^2, Phi(h), Phi(-h)
};

// Phi(hmax) - Phi(hmin): upper tails where hmax > 0, lower tails otherwise (the difference of the two small numbers)
__device__ __forceinline__ double pb_phi_diff(const PbCurve &lo, const PbCurve &hi) {
    return hi.h > 0.0 ? lo.Q - hi.Q : hi.P - lo.P;
}

// Drezner-Wesolowsky sum of BVND over L node pairs
template <int L>
__device__ __forceinline__ double pb_dw_sum(const double *X, const double *W, double asr, double hk, double hs) {
    double s = 0.0;
#pragma unroll 1
    for (int i = 0; i < L; ++i) {
        double sn = sin(asr * (X[i] + 1.0) * 0.5);
        s += W[i] * exp((sn * hk - hs) / (1.0 - sn * sn));
        sn = sin(asr * (1.0 - X[i]) * 0.5);
        s += W[i] * exp((sn * hk - hs) / (1.0 - sn * sn));
    }
    return s;
}

// p for one (pair, timepoint); point_i: sigma_i = 0
__device__ double pb_prob(bool point_i, const PbCurve &J, const PbCurve &K) {
    if (point_i) {
        const double ej = J.u == 0.0 ? 1.0 - J.P - J.Q : 0.0;      // point masses: exact indicators
        const double ek = K.u == 0.0 ? 1.0 - K.P - K.Q : 0.0;
        return J.Q * K.P + J.P * K.Q + ej + ek - ej * ek;
    }
    const bool jlo = J.h <= K.h;
    const PbCurve &lo = jlo ? J : K, &hi = jlo ? K : J;
    if (J.u == 0.0 && K.u == 0.0) return pb_phi_diff(lo, hi);
    const double rho = J.g * K.g;
    const double hk = J.h * K.h;
    if (rho < 0.925) {
        const double asr = asin(rho), hs = 0.5 * (J.h * J.h + K.h * K.h);
        double s;
        if (rho < 0.3)
            s = pb_dw_sum<3>(PB_GL6_X, PB_GL6_W, asr, hk, hs);
        else if (rho < 0.75)
            s = pb_dw_sum<6>(PB_GL12_X, PB_GL12_W, asr, hk, hs);
        else
            s = pb_dw_sum<10>(PB_GL20_X, PB_GL20_W, asr, hk, hs);
        return J.P * K.Q + J.Q * K.P - s * asr / (2.0 * M_PI);
    }
    // Genz's |r| >= 0.925 branch for r = -rho (its k -> -k flip makes hk = h_j h_k, bs = (h_j - h_k)^2 for both orthants)
    const double as = J.u + J.g * J.g * K.u;                        // 1 - rho^2 > 0 (not both u zero)
    const double bs = (J.h - K.h) * (J.h - K.h);
    double a = sqrt(as);
    const double c = (4.0 - hk) / 8.0, d = (12.0 - hk) / 16.0;
    double bvn = 0.0;
    double asr = -(bs / as + hk) * 0.5;
    if (asr > -100.0) bvn = a * exp(asr) * (1.0 - c * (bs - as) * (1.0 - d * bs / 5.0) / 3.0 + c * d * as * as / 5.0);
    const double e = exp(-hk * 0.5);
    if (-hk < 100.0 && e > 0.0) {
        const double b = sqrt(bs);
        bvn -= e * sqrt(2.0 * M_PI) * pr_phi(-b / a) * b * (1.0 - c * bs * (1.0 - d * bs / 5.0) / 3.0);
    }
    a *= 0.5;
#pragma unroll 1
    for (int i = 0; i < 10; ++i) {
#pragma unroll 1
        for (int sg = 0; sg < 2; ++sg) {
            const double x = sg ? 1.0 - PB_GL20_X[i] : 1.0 + PB_GL20_X[i];
            const double xs = (a * x) * (a * x);
            const double rs = sqrt(1.0 - xs);
            asr = -(bs / xs + hk) * 0.5;
            if (asr > -100.0)
                bvn += a * PB_GL20_W[i] * exp(asr) *
                       (exp(-hk * xs / (2.0 * (1.0 + rs) * (1.0 + rs))) / rs - (1.0 + c * xs * (1.0 + d * xs)));
        }
    }
    return bvn / M_PI + pb_phi_diff(lo, hi);
}

// grid: units u0 .. u0 + gridDim.x - 1, timepoints [t0, t1).  Unit u = (target q = u / S, tile u % S = (ab, bb), ab <= bb
// in row-major order over the nb x nb upper triangle).  Position p of target q is column members[q][p] (or p), skipped
// where it is -1, out of range or the target.  first: start the pair values; last: reduce them into part[blockIdx.x];
// otherwise they go to st for the next launch.
template <bool RELAX>
__global__ __launch_bounds__(PB_THREADS) void pb_kernel(const double *__restrict__ mu, const double *__restrict__ var, i64 n,
                                                         const i64 *__restrict__ targets, const int *__restrict__ members,
                                                         i64 bs, i64 W, i64 nb, u64 S, u64 u0, i64 t0, i64 t1, int first,
                                                         int last, double *__restrict__ st, double *__restrict__ part) {
    __shared__ PbCurve sc[PB_TC][2 * PB_B];
    __shared__ double sacc[PB_PAIRS][PB_THREADS];
    __shared__ int scol[2 * PB_B];
    __shared__ int spoint[PB_TC];
    __shared__ double scratch[4];
    const int tid = threadIdx.x;
    const u64 u = u0 + blockIdx.x;
    const i64 q = (i64)(u / S);
    i64 r = (i64)(u % S), ab = 0, len = nb;
    while (r >= len) {
        r -= len;
        ++ab;
        --len;
    }
    const i64 bb = ab + r;
    const i64 i = targets ? targets[q] : q;
    if (tid < 2 * PB_B) {
        const i64 pos = (tid < PB_B ? ab : bb) * PB_B + (tid & (PB_B - 1));
        i64 col = -1;
        if (pos < W) col = members ? (i64)members[q * bs + pos] : pos;
        scol[tid] = (col >= 0 && col < n && col != i) ? (int)col : -1;
    }
    __syncthreads();
    const int a = tid & (PB_B - 1), bw = tid >> 6;
    unsigned vmask = 0;
    if (scol[a] >= 0)
        for (int s = 0; s < PB_PAIRS; ++s) {
            const int b = bw + 4 * s;
            if (scol[PB_B + b] >= 0 && (ab != bb || a < b)) vmask |= 1u << s;
        }
    for (int s = 0; s < PB_PAIRS; ++s)
        sacc[s][tid] = first ? (RELAX ? 0.0 : (double)((vmask >> s) & 1u)) : st[((u64)blockIdx.x * PB_PAIRS + s) * PB_THREADS + tid];
    for (i64 tc = t0; tc < t1; tc += PB_TC) {
        if (!RELAX) {                                               // every product of the tile exactly 0: done
            int alive = 0;
            for (int s = 0; s < PB_PAIRS; ++s) alive |= sacc[s][tid] != 0.0;
            if (!__syncthreads_or(alive)) break;
        }
        for (int e = tid; e < 2 * PB_B * PB_TC; e += PB_THREADS) {
            const int sl = e % (2 * PB_B), tt = e / (2 * PB_B);
            const i64 t = tc + tt;
            const int col = scol[sl];
            if (t >= t1) continue;
            const double mi = mu[t * n + i], vi = var[t * n + i];
            if (sl == 0) spoint[tt] = vi == 0.0;
            if (col < 0) continue;
            const double d = mi - mu[t * n + col];
            const double si = sqrt(vi), sk = sqrt(var[t * n + col]);
            const double s = hypot(si, sk);
            PbCurve c;
            if (s == 0.0) {                                         // two point masses
                c = PbCurve{0.0, 0.0, 0.0, d > 0.0 ? 1.0 : 0.0, d < 0.0 ? 1.0 : 0.0};
            } else {
                const double rs = 1.0 / s;
                const double h = fmin(fmax(d * rs, -PB_HMAX), PB_HMAX);
                const double w = sk * rs;
                c = PbCurve{h, si * rs, w * w, pr_phi(h), pr_phi(-h)};
            }
            sc[tt][sl] = c;
        }
        __syncthreads();
        const int nt = t1 - tc < PB_TC ? (int)(t1 - tc) : PB_TC;
        if (vmask)
            for (int tt = 0; tt < nt; ++tt) {
                const PbCurve A = sc[tt][a];
                const bool pi = spoint[tt] != 0;
#pragma unroll 1
                for (int s = 0; s < PB_PAIRS; ++s) {
                    if (!((vmask >> s) & 1u)) continue;
                    const double cur = sacc[s][tid];
                    if (!RELAX && cur == 0.0) continue;
                    const double p = pb_prob(pi, A, sc[tt][PB_B + bw + 4 * s]);
                    sacc[s][tid] = RELAX ? cur + p : cur * p;
                }
            }
        __syncthreads();
    }
    if (last) {
        double v = 0.0;
        for (int s = 0; s < PB_PAIRS; ++s) v += sacc[s][tid];
        const double tot = pr_block_sum(v, scratch);
        if (tid == 0) part[blockIdx.x] = tot;
    } else {
        for (int s = 0; s < PB_PAIRS; ++s) st[((u64)blockIdx.x * PB_PAIRS + s) * PB_THREADS + tid] = sacc[s][tid];
    }
}

int launch_prob_band_sums(const double *mu, const double *var, i64 T, i64 n, const i64 *targets, i64 m, const int *members,
                          int bs, int relax, double *out, hipStream_t s) {
    const i64 W = members ? (i64)bs : n;
    const i64 nb = (W + PB_B - 1) / PB_B;
    const u64 S = (u64)nb * (u64)(nb + 1) / 2;
    if (S == 0) {                                                   // no position: no pair
        SD_HIP(hipMemsetAsync(out, 0, sizeof(double) * m, s));
        return SD_OK;
    }
    const u64 units = (u64)m * S;
    const u64 Tn = T > 0 ? (u64)T : 1;
    // units per launch G and timepoints per launch tl: whole timelines while G can still fill the GPU
    u64 G = PB_LAUNCH_EVALS / (PB_TILE * Tn), tl = Tn;
    if (G < PB_MIN_UNITS) {
        G = PB_MIN_UNITS;
        tl = PB_LAUNCH_EVALS / (PB_TILE * G);
        if (tl < 1) tl = 1;
    }
    const long long forced = xswitch("SD_PROB_LAUNCH_UNITS");     // cross-check build only: units AND timepoints per launch
    if (forced > 0) G = tl = (u64)forced;
    if (G > units) G = units;
    if (tl > Tn) tl = Tn;
    if (G > 0x7fffffff) G = 0x7fffffff;
    const bool split = tl < (u64)T;
    const size_t part_b = align_up(G * sizeof(double), 256);
    const size_t st_b = split ? G * PB_PAIRS * PB_THREADS * sizeof(double) : 0;
    char *ws = nullptr;
    SD_HIP(hipMallocAsync((void **)&ws, part_b + st_b, s));
    double *part = (double *)ws, *st = split ? (double *)(ws + part_b) : nullptr;
    hipError_t err = hipSuccess;
    for (u64 u0 = 0; u0 < units && err == hipSuccess; u0 += G) {
        const u64 cnt = units - u0 < G ? units - u0 : G;
        i64 t0 = 0;
        do {
            const i64 t1 = (u64)(T - t0) < tl ? T : t0 + (i64)tl;
            const int first = t0 == 0, last = t1 >= T;
            if (relax)
                hipLaunchKernelGGL(pb_kernel<true>, dim3((unsigned)cnt), dim3(PB_THREADS), 0, s, mu, var, n, targets, members,
                                   (i64)bs, W, nb, S, u0, t0, t1, first, last, st, part);
            else
                hipLaunchKernelGGL(pb_kernel<false>, dim3((unsigned)cnt), dim3(PB_THREADS), 0, s, mu, var, n, targets, members,
                                   (i64)bs, W, nb, S, u0, t0, t1, first, last, st, part);
            if ((err = hipGetLastError()) != hipSuccess) break;
            t0 = t1;
        } while (t0 < T);
        if (err != hipSuccess) break;
        err = launch_prob_fold(part, u0, u0 + cnt, S, out, s);
    }
    const hipError_t ferr = hipFreeAsync(ws, s);
    if (err != hipSuccess)
        return fail(SD_ERR_HIP, "probabilistic band launch failed: %s (%s:%d)", hipGetErrorString(err), __FILE__, __LINE__);
    SD_HIP(ferr);
    return SD_OK;
}

}  // namespace sd
