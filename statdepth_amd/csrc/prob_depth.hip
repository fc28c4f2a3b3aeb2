// prob_depth.hip -- K8: probabilistic depths of normal distributions and of Poisson curves.
//
// Normal (replaces _normal_depth, _uncertainty.py:101-121: one scipy quad per (target, pair)).  The reference integrates
// (Phi_i - Phi_k Phi_j) phi_k over every pair i < j of the target k's others.  With X_m ~ N(mu_m, sigma_m),
// s = sqrt(sigma_m^2 + sigma_k^2) and h = (mu_k - mu_m) / s the two integrals are closed forms:
//   A(m, k) = int Phi_m phi_k     = Phi(h)
//   B(k, m) = int Phi_k Phi_m phi_k = Phi2(0, h; rho) = Phi(h) / 2 + T(h, a),  rho = sigma_k / (sqrt(2) s) < 1/sqrt(2),
//                                     a = rho / sqrt(1 - rho^2) = sigma_k / sqrt(2 sigma_m^2 + sigma_k^2) < 1,
// T being Owen's T, here by 12-point Gauss-Legendre on [0, a] (its integrand is smooth and a < 1).  A pair term A - B is
// within 9.1e-17 absolute of its 40-digit value for every h (0, 1e-300 ... 1e5, inf) and every a (1e-150 ... 1), measured on
// an MI355X; tests/test_prob_pairs_gpu.py holds 3.7e-16.  The bound is absolute: T keeps no relative accuracy where it
// is small (2e-5 relative at h = 12, a -> 1, a CPU measurement).  h and a are ratios, so the means of a pair are scaled
// by 2^-4 where one exceeds 2^1020, its stds by 2^-4 where one exceeds 2^1020 and by 2^106 where both are below 2^-969
// (pn_kernel): every finite input with positive stds gives a finite output, subnormal stds beside 1e308 means included.
// Counting how often each one appears in the pairs:
//   out[q] = sum_{m != k} A(m, k) ((n - 1 - m) - [k > m])  -  sum_{m != k} B(k, m) (m - [k < m]),   k = targets[q]
// O(n) per target.  A workgroup takes one (target, chunk of PN_CHUNK partners) unit; each lane keeps the two weighted sums in
// fp64, the workgroup reduces them in a fixed tree and writes their difference; pn_fold_kernel adds a target's chunks in
// chunk order.  No atomics: a target's bits depend neither on the other targets nor on how the call is cut into launches.
//
// Poisson (replaces _poisson_depth / _poisson_containment_simplified, _uncertainty.py:34-61).  For rates lam[t][c], with
// p_c(z) = P(X_c = z), L_c(z) = P(X_c <= z), U_c(z) = P(X_c >= z), the reference's sum for target f is
//   out[f] = sum_t sum_{z=1}^{lim-1} p_f(z) S_f(t, z),   S_f = sum over column pairs i < j, both != f, of L_i U_j
// (orientation kept: i is the earlier column).  Over the columns in order, the triple (sum L, sum U, sum_{i<j} L_i U_j) of
// a run of columns composes associatively: (a then b) = (a.L + b.L, a.U + b.U, a.P + b.P + a.L b.U).  So with A the
// triple of the columns before f and B that of the columns after f, S_f = A.P + B.P + A.L B.U -- sums of non-negative
// terms only.  Per (t, z) the columns are scanned on chip in blocks of 256 (one column per lane):
//   pp_useed_kernel   per (t, column): U at the end of every chunk of PP_Z values of z, by a backward running sum
//   pp_block_kernel<0> per (t, column block): every z, the block's triple (block scan)        -> agg
//   pp_scan_kernel    per (t, z): exclusive scans of the block triples, both directions         -> pre, suf
//   pp_block_kernel<1> per (t, column block): every z, S_f from the in-block scans and pre/suf; a lane sums p_f S_f
//                                             over z for its own column                         -> part[t][f]
//   pp_fold_kernel    per target: part summed over t in order, carried in out between launches
// Scratch is O(T_launch (n lim / PP_Z + lim n / 256)): the T x n x lim intermediates never exist.
// p is Loader's saddle-point form exp(-stirlerr(z) - bd0(z, lam)) / sqrt(2 pi z) (no lam^z, no z!), seeded at each
// chunk start and carried by p(z + 1) = p(z) (lam / (z + 1)) for at most PP_Z - 1 steps.  L is a forward running sum from
// L(0) = e^-lam; U a backward running sum from the chunk-end seeds, themselves a backward running sum from U(lim) (see
// pp_tail).  Every z of 1 .. lim - 1 is evaluated: nothing is cut short.  Against exact sums (n = 3, T = 1, 40 digits;
// tests/test_prob_pairs_gpu.py, rtol 1e-12) the worst relative errors measured on an MI355X are 2.5e-15 / 1.8e-15 /
// 6.6e-15 / 1.1e-15 at stirlerr's seams z = 15|16, 35|36, 80|81, 500|501, 1.1e-14 at bd0's series switch, 1.1e-14 at
// pp_tail's lam = lim branch and re-seeds, 2.4e-14 at the 16-z chunk edges of lim.
//
// fp64 VALU and transcendentals (erfc, exp, log) are the hot path; the guides give no fp64 rate for this part, so the
// costs in DESIGN §3 K8 are measured, not derived from a peak.
#include "prob_common.h"

namespace sd {

// ---------------------------------------------------------------------------------------------------------------- normal
constexpr int PN_THREADS = 256;
constexpr int PN_PER_THREAD = 8;
constexpr i64 PN_CHUNK = (i64)PN_THREADS * PN_PER_THREAD;          // partners per workgroup
// pairs per launch: 2^30, i.e. 2^19 workgroups (the n = 10^5 case is ~10 launches)
constexpr u64 PN_LAUNCH_UNITS = ((u64)1 << 30) / PN_CHUNK;

// 12-point Gauss-Legendre on [-1, 1]: the positive nodes and their weights
__constant__ double GL12_X[6] = {0.1252334085114689, 0.3678314989981802, 0.5873179542866175,
                                 0.7699026741943047, 0.9041172563704748, 0.9815606342467192};
__constant__ double GL12_W[6] = {0.2491470458134027, 0.23349253653835464, 0.20316742672306565,
                                 0.1600783285433461, 0.10693932599531888, 0.04717533638651202};

// Owen's T(h, a) = (1 / 2 pi) int_0^a exp(-h^2 (1 + x^2) / 2) / (1 + x^2) dx, 0 <= a < 1
__device__ __forceinline__ double pn_owen_t(double h, double a) {
    const double hh = 0.5 * h * h;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double x1 = 0.5 * a * (1.0 - GL12_X[i]), x2 = 0.5 * a * (1.0 + GL12_X[i]);
        const double q1 = 1.0 + x1 * x1, q2 = 1.0 + x2 * x2;
        s += GL12_W[i] * (exp(-hh * q1) / q1 + exp(-hh * q2) / q2);
    }
    return s * (0.25 * a / M_PI);
}

// unit u = u0 + blockIdx.x = (target q = u / S, chunk c = u % S); part[blockIdx.x] = the chunk's A-sum minus its B-sum
__global__ __launch_bounds__(PN_THREADS) void pn_kernel(const double *__restrict__ mu, const double *__restrict__ sg, i64 n,
                                                         const i64 *__restrict__ targets, u64 u0, u64 S,
                                                         double *__restrict__ part) {
    __shared__ double scratch[4];
    const u64 u = u0 + blockIdx.x;
    const i64 q = (i64)(u / S);
    const i64 c = (i64)(u % S);
    const i64 k = targets ? targets[q] : q;
    const double mk = mu[k], sk = sg[k];
    double sa = 0.0, sb = 0.0;
#pragma unroll 2
    for (int j = 0; j < PN_PER_THREAD; ++j) {
        const i64 m = c * PN_CHUNK + (i64)j * PN_THREADS + threadIdx.x;
        if (m < n && m != k) {
            const double mm = mu[m], smax = fmax(sg[m], sk);
            // h and a are ratios, so the means and the stds each take a power of two of their own (exact; 1 in between,
            // where every bit stays as it was) and h gets the quotient back: cm keeps the difference finite, cs keeps
            // sqrt(2) sm and the hypots finite at the top of the range and the subnormal stds' bits at its bottom.  A
            // partner that the small factor pushes below the subnormals is beyond 2^-2000 of the other: no digit of it counts
            const double cm = fmax(fabs(mk), fabs(mm)) > 0x1p1020 ? 0x1p-4 : 1.0;
            const double cs = smax > 0x1p1020 ? 0x1p-4 : (smax < 0x1p-969 ? 0x1p106 : 1.0);
            const double sm = sg[m] * cs, skk = sk * cs;
            const double h = (mk * cm - mm * cm) / hypot(sm, skk) * (cs / cm);
            const double Ph = pr_phi(h);
            const double a = skk / hypot(M_SQRT2 * sm, skk);
            const double B = 0.5 * Ph + pn_owen_t(h, a);
            const double wa = (double)((n - 1 - m) - (k > m ? 1 : 0));
            const double wb = (double)(m - (k < m ? 1 : 0));
            sa += Ph * wa;
            sb += B * wb;
        }
    }
    const double ta = pr_block_sum(sa, scratch);
    const double tb = pr_block_sum(sb, scratch);
    if (threadIdx.x == 0) part[blockIdx.x] = ta - tb;
}

// add the chunk results of units [u0, u1) into out[q] in chunk order (out holds the running sum between launches)
__global__ __launch_bounds__(256) void pn_fold_kernel(const double *__restrict__ part, u64 u0, u64 u1, u64 S,
                                                      double *__restrict__ out) {
    const i64 q = (i64)(u0 / S) + (i64)blockIdx.x * 256 + threadIdx.x;
    const u64 qb = (u64)q * S, qe = qb + S;
    if (qb >= u1) return;
    const u64 a = qb > u0 ? qb : u0, e = qe < u1 ? qe : u1;
    double acc = a == qb ? 0.0 : out[q];
    for (u64 v = a; v < e; ++v) acc += part[v - u0];
    out[q] = acc;
}

// the fold above as a stream launch of its own (K9's per-(target, tile) results use it too)
hipError_t launch_prob_fold(const double *part, u64 u0, u64 u1, u64 S, double *out, hipStream_t s) {
    const u64 q0 = u0 / S, q1 = (u1 - 1) / S;
    hipLaunchKernelGGL(pn_fold_kernel, dim3((unsigned)((q1 - q0 + 1 + 255) / 256)), dim3(256), 0, s, part, u0, u1, S, out);
    return hipGetLastError();
}

int launch_prob_normal_sums(const double *mu, const double *sigma, i64 n, const i64 *targets, i64 m, double *out,
                            hipStream_t s) {
    const u64 S = (u64)((n + PN_CHUNK - 1) / PN_CHUNK);
    const u64 units = (u64)m * S;
    u64 per_launch = PN_LAUNCH_UNITS;
    const long long forced = xswitch("SD_PROB_LAUNCH_UNITS");     // cross-check build only: force launch splits
    if (forced > 0) per_launch = (u64)forced;
    if (per_launch > units) per_launch = units;
    double *part = nullptr;
    SD_HIP(hipMallocAsync((void **)&part, per_launch * sizeof(double), s));
    hipError_t err = hipSuccess;
    for (u64 u0 = 0; u0 < units && err == hipSuccess; u0 += per_launch) {
        const u64 cnt = units - u0 < per_launch ? units - u0 : per_launch;
        hipLaunchKernelGGL(pn_kernel, dim3((unsigned)cnt), dim3(PN_THREADS), 0, s, mu, sigma, n, targets, u0, S, part);
        err = hipGetLastError();
        if (err != hipSuccess) break;
        const u64 q0 = u0 / S, q1 = (u0 + cnt - 1) / S;
        hipLaunchKernelGGL(pn_fold_kernel, dim3((unsigned)((q1 - q0 + 1 + 255) / 256)), dim3(256), 0, s, part, u0, u0 + cnt,
                           S, out);
        err = hipGetLastError();
    }
    const hipError_t ferr = hipFreeAsync(part, s);
    if (err != hipSuccess)
        return fail(SD_ERR_HIP, "probabilistic normal launch failed: %s (%s:%d)", hipGetErrorString(err), __FILE__, __LINE__);
    SD_HIP(ferr);
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------------------------- Poisson
constexpr int PP_THREADS = 256;                                     // columns per block
constexpr int PP_Z = 16;                                            // z values per chunk (p and U held in registers)
// (t, column, z) evaluations per launch: 2^30 (a launch covers whole rows t; at least one)
constexpr u64 PP_LAUNCH_EVALS = (u64)1 << 30;
constexpr u64 PP_SCRATCH_BYTES = (u64)512 << 20;                  // per launch, unless one row alone needs more

struct Tri {
    double l, u, p;                                                 // sum L, sum U, sum over i < j of L_i U_j
};
__device__ __forceinline__ Tri tri_cat(const Tri &a, const Tri &b) {
    return Tri{a.l + b.l, a.u + b.u, a.p + b.p + a.l * b.u};
}
__device__ __forceinline__ Tri tri_shfl_up(const Tri &x, int o) {
    return Tri{__shfl_up(x.l, o), __shfl_up(x.u, o), __shfl_up(x.p, o)};
}
__device__ __forceinline__ Tri tri_shfl_down(const Tri &x, int o) {
    return Tri{__shfl_down(x.l, o), __shfl_down(x.u, o), __shfl_down(x.p, o)};
}

// Loader's Stirling-formula error, stirlerr(z) = lgamma(z + 1) - (z + 1/2) log z + z - log sqrt(2 pi), integer z >= 1
__device__ __forceinline__ double pp_stirlerr(double z) {
    if (z <= 15.0) {
        const double tab[16] = {0.0, 0.08106146679532726, 0.0413406959554093, 0.02767792568499834, 0.020790672103765093,
                                0.016644691189821193, 0.013876128823070748, 0.01189670994589177, 0.010411265261972096,
                                0.009255462182712733, 0.00833056343336287, 0.007573675487951841, 0.00694284010720953,
                                0.006408994188004207, 0.0059513701127588475, 0.005554733551962801};
        return tab[(int)z];
    }
    const double S0 = 1.0 / 12, S1 = 1.0 / 360, S2 = 1.0 / 1260, S3 = 1.0 / 1680, S4 = 1.0 / 1188;
    const double zz = z * z;
    if (z > 500) return (S0 - S1 / zz) / z;
    if (z > 80) return (S0 - (S1 - S2 / zz) / zz) / z;
    if (z > 35) return (S0 - (S1 - (S2 - S3 / zz) / zz) / zz) / z;
    return (S0 - (S1 - (S2 - (S3 - S4 / zz) / zz) / zz) / zz) / z;
}

// Loader's deviance term bd0(x, l) = x log(x / l) + l - x, by its series where x is near l (no cancellation)
__device__ __forceinline__ double pp_bd0(double x, double l) {
    if (fabs(x - l) < 0.1 * (x + l)) {
        double v = (x - l) / (x + l);
        double s = (x - l) * v;
        double ej = 2.0 * x * v;
        v = v * v;
        for (int j = 1; j < 1000; ++j) {
            ej *= v;
            const double s1 = s + ej / (double)(2 * j + 1);
            if (s1 == s) return s1;
            s = s1;
        }
        return s;
    }
    return x * log(x / l) + l - x;
}

// P(X = z) for integer z >= 1 and lam >= 0
__device__ __forceinline__ double pp_dpois(double z, double lam) {
    if (lam == 0.0) return 0.0;
    return exp(-pp_stirlerr(z) - pp_bd0(z, lam)) / sqrt(2.0 * M_PI * z);
}

// p(z0 .. z0 + len - 1): seeded at the chunk start, then the ratio recurrence (the same ops in every kernel: same bits)
__device__ __forceinline__ void pp_chunk_pmf(double lam, i64 z0, int len, double (&p)[PP_Z]) {
    p[0] = pp_dpois((double)z0, lam);
#pragma unroll
    for (int k = 1; k < PP_Z; ++k) p[k] = k < len ? p[k - 1] * (lam / (double)(z0 + k)) : 0.0;
}

// U(lim) = P(X >= lim), lim >= 2.  Where lim > lam it is the upper tail, summed upward (terms fall; stopped once the
// remainder, at most p r / (1 - r) with r = lam / (k + 1), is below 2^-56 of the sum).  Where lim <= lam it is above 1/2:
// 1 - P(X <= lim - 1), the lower tail below 1/2 (lim - 1 < lam - ln 2 <= the median) summed downward the same way, so the
// difference loses no digit.  The ratio recurrence is re-seeded every 32 terms.
__device__ double pp_tail(i64 lim, double lam) {
    if (lam == 0.0) return 0.0;
    if (!(lam > 0.0)) return lam;                                  // NaN (the host refuses it): no loop on it
    const double tiny = 1.0 / 72057594037927936.0;                  // 2^-56
    double s = 0.0;
    if ((double)lim > lam) {
        i64 k = lim;
        double p = pp_dpois((double)k, lam);
        for (;;) {
            s += p;
            const double r = lam / (double)(k + 1);
            if (!(p > 0.0) || p * r <= s * (1.0 - r) * tiny) break;   // (p == 0: every later term is 0)
            ++k;
            p = ((k - lim) & 31) == 0 ? pp_dpois((double)k, lam) : p * r;
        }
        return s;
    }
    i64 k = lim - 1;
    double p = pp_dpois((double)k, lam);
    for (;;) {
        s += p;
        if (k == 0) break;
        const double r = (double)k / lam;
        if (p * r <= s * (1.0 - r) * tiny) break;
        --k;
        p = k == 0 ? exp(-lam) : (((lim - 1 - k) & 31) == 0 ? pp_dpois((double)k, lam) : p * r);
    }
    return 1.0 - s;
}

// one thread per (row tt of the launch, column c): useed[(tt * nch + b) * n + c] = U(end of chunk b)
__global__ __launch_bounds__(256) void pp_useed_kernel(const double *__restrict__ lam, i64 n, i64 lim, i64 t0, i64 tl, i64 nch,
                                                       double *__restrict__ useed) {
    const i64 g = (i64)blockIdx.x * 256 + threadIdx.x;
    if (g >= tl * n) return;
    const i64 tt = g / n, c = g % n;
    const double l = lam[(t0 + tt) * n + c];
    double U = pp_tail(lim, l);
    for (i64 b = nch - 1; b >= 0; --b) {
        const i64 z0 = 1 + b * PP_Z;
        const int len = (int)(lim - z0 < PP_Z ? lim - z0 : PP_Z);
        useed[(tt * nch + b) * n + c] = U;
        double p[PP_Z];
        pp_chunk_pmf(l, z0, len, p);
#pragma unroll
        for (int k = PP_Z - 1; k >= 0; --k)
            if (k < len) U += p[k];
    }
}

// grid (column block b, row tt).  MODE 0: agg[(tt * nz + z - 1) * nb + b] = the block's triple at z.
// MODE 1: part[tt * n + c] = sum_z p_c(z) S_c(z), with pre / suf the triples of the columns before / after block b.
template <int MODE>
__global__ __launch_bounds__(PP_THREADS) void pp_block_kernel(const double *__restrict__ lam, i64 n, i64 lim, i64 t0, i64 nch,
                                                              const double *__restrict__ useed, Tri *__restrict__ agg,
                                                              const Tri *__restrict__ pre, const Tri *__restrict__ suf,
                                                              double *__restrict__ part) {
    __shared__ Tri wf[2][4], wb[2][4];
    const i64 nb = gridDim.x, b = blockIdx.x, tt = blockIdx.y;
    const i64 nz = lim - 1;
    const i64 c = b * PP_THREADS + threadIdx.x;
    const bool on = c < n;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double l = on ? lam[(t0 + tt) * n + c] : 0.0;
    double L = on ? exp(-l) : 0.0;                                  // L(0)
    double acc = 0.0;
    int par = 0;
    for (i64 ch = 0; ch < nch; ++ch) {
        const i64 z0 = 1 + ch * PP_Z;
        const int len = (int)(lim - z0 < PP_Z ? lim - z0 : PP_Z);
        double p[PP_Z], U[PP_Z];
        pp_chunk_pmf(l, z0, len, p);
        double u = on ? useed[(tt * nch + ch) * n + c] : 0.0;
#pragma unroll
        for (int k = PP_Z - 1; k >= 0; --k) {
            if (k < len) u += p[k];
            U[k] = u;
        }
#pragma unroll
        for (int k = 0; k < PP_Z; ++k) {
            if (k >= len) continue;                                 // uniform across the block
            L += p[k];
            const Tri x = on ? Tri{L, U[k], 0.0} : Tri{0.0, 0.0, 0.0};
            Tri f = x;                                              // inclusive forward scan in the wave
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const Tri y = tri_shfl_up(f, o);
                if (lane >= o) f = tri_cat(y, f);
            }
            if (lane == 63) wf[par][w] = f;
            Tri g = x;                                              // inclusive backward scan in the wave
            if constexpr (MODE == 1) {
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const Tri y = tri_shfl_down(g, o);
                    if (lane + o < 64) g = tri_cat(g, y);
                }
                if (lane == 0) wb[par][w] = g;
            }
            __syncthreads();                                        // double-buffered by par: one barrier per z
            const i64 zi = (tt * nz + (z0 + k - 1)) * nb + b;
            if constexpr (MODE == 0) {
                if (threadIdx.x == 0) {
                    Tri t = wf[par][0];
                    for (int v = 1; v < 4; ++v) t = tri_cat(t, wf[par][v]);
                    agg[zi] = t;
                }
            } else {
                Tri A = pre[zi];                                    // the columns before this one
                for (int v = 0; v < w; ++v) A = tri_cat(A, wf[par][v]);
                const Tri fe = tri_shfl_up(f, 1);
                if (lane > 0) A = tri_cat(A, fe);
                Tri B = suf[zi];                                    // the columns after this one
                for (int v = 3; v > w; --v) B = tri_cat(wb[par][v], B);
                const Tri ge = tri_shfl_down(g, 1);
                if (lane < 63) B = tri_cat(ge, B);
                acc += p[k] * (A.p + B.p + A.l * B.u);
            }
            par ^= 1;
        }
    }
    if constexpr (MODE == 1)
        if (on) part[tt * n + c] = acc;
}

// one thread per (row tt, z): pre[b] = triple of blocks 0 .. b - 1, suf[b] = triple of blocks b + 1 .. nb - 1
__global__ __launch_bounds__(256) void pp_scan_kernel(const Tri *__restrict__ agg, i64 rows, i64 nb, Tri *__restrict__ pre,
                                                      Tri *__restrict__ suf) {
    const i64 g = (i64)blockIdx.x * 256 + threadIdx.x;
    if (g >= rows) return;
    const Tri *a = agg + g * nb;
    Tri r{0.0, 0.0, 0.0};
    for (i64 b = 0; b < nb; ++b) {
        pre[g * nb + b] = r;
        r = tri_cat(r, a[b]);
    }
    r = Tri{0.0, 0.0, 0.0};
    for (i64 b = nb - 1; b >= 0; --b) {
        suf[g * nb + b] = r;
        r = tri_cat(a[b], r);
    }
}

__global__ __launch_bounds__(256) void pp_fold_kernel(const double *__restrict__ part, i64 n, i64 tl, const i64 *__restrict__ targets,
                                                      i64 m, int first, double *__restrict__ out) {
    const i64 q = (i64)blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    const i64 c = targets ? targets[q] : q;
    double acc = first ? 0.0 : out[q];
    for (i64 tt = 0; tt < tl; ++tt) acc += part[tt * n + c];
    out[q] = acc;
}

int launch_prob_poisson_sums(const double *lam, i64 T, i64 n, i64 lim, const i64 *targets, i64 m, double *out, hipStream_t s) {
    const i64 nz = lim - 1;
    if (nz <= 0 || T == 0 || n < 3) {                               // no z, no row or no pair: empty sums
        SD_HIP(hipMemsetAsync(out, 0, sizeof(double) * m, s));
        return SD_OK;
    }
    const i64 nch = (nz + PP_Z - 1) / PP_Z;
    const i64 nb = (n + PP_THREADS - 1) / PP_THREADS;
    // bytes per row of a launch: U seeds, block triples (agg, pre, suf) and the per-column results
    const u64 row_bytes = (u64)nch * n * sizeof(double) + 3 * (u64)nz * nb * sizeof(Tri) + (u64)n * sizeof(double);
    i64 tl = (i64)(PP_LAUNCH_EVALS / ((u64)n * (u64)nz));
    if ((u64)tl * row_bytes > PP_SCRATCH_BYTES) tl = (i64)(PP_SCRATCH_BYTES / row_bytes);
    const long long forced = xswitch("SD_PROB_LAUNCH_UNITS");     // cross-check build only: rows per launch
    if (forced > 0) tl = forced;
    if (tl < 1) tl = 1;
    if (tl > T) tl = T;
    if (tl > 65535) tl = 65535;                                     // grid.y
    if (nb > 0x7fffffff) return fail(SD_ERR_UNSUPPORTED, "too many columns");
    char *ws = nullptr;
    const size_t useed_b = align_up((size_t)tl * nch * n * sizeof(double), 256);
    const size_t tri_b = align_up((size_t)tl * nz * nb * sizeof(Tri), 256);
    const size_t part_b = align_up((size_t)tl * n * sizeof(double), 256);
    SD_HIP(hipMallocAsync((void **)&ws, useed_b + 3 * tri_b + part_b, s));
    double *useed = (double *)ws;
    Tri *agg = (Tri *)(ws + useed_b), *pre = (Tri *)(ws + useed_b + tri_b), *suf = (Tri *)(ws + useed_b + 2 * tri_b);
    double *part = (double *)(ws + useed_b + 3 * tri_b);
    hipError_t err = hipSuccess;
    for (i64 t0 = 0; t0 < T && err == hipSuccess; t0 += tl) {
        const i64 rows = T - t0 < tl ? T - t0 : tl;
        hipLaunchKernelGGL(pp_useed_kernel, dim3((unsigned)((rows * n + 255) / 256)), dim3(256), 0, s, lam, n, lim, t0, rows, nch,
                           useed);
        if ((err = hipGetLastError()) != hipSuccess) break;
        hipLaunchKernelGGL(pp_block_kernel<0>, dim3((unsigned)nb, (unsigned)rows), dim3(PP_THREADS), 0, s, lam, n, lim, t0, nch,
                           useed, agg, (const Tri *)nullptr, (const Tri *)nullptr, (double *)nullptr);
        if ((err = hipGetLastError()) != hipSuccess) break;
        hipLaunchKernelGGL(pp_scan_kernel, dim3((unsigned)((rows * nz + 255) / 256)), dim3(256), 0, s, agg, rows * nz, nb, pre,
                           suf);
        if ((err = hipGetLastError()) != hipSuccess) break;
        hipLaunchKernelGGL(pp_block_kernel<1>, dim3((unsigned)nb, (unsigned)rows), dim3(PP_THREADS), 0, s, lam, n, lim, t0, nch,
                           useed, (Tri *)nullptr, pre, suf, part);
        if ((err = hipGetLastError()) != hipSuccess) break;
        hipLaunchKernelGGL(pp_fold_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, part, n, rows, targets, m,
                           t0 == 0 ? 1 : 0, out);
        err = hipGetLastError();
    }
    const hipError_t ferr = hipFreeAsync(ws, s);
    if (err != hipSuccess)
        return fail(SD_ERR_HIP, "probabilistic Poisson launch failed: %s (%s:%d)", hipGetErrorString(err), __FILE__, __LINE__);
    SD_HIP(ferr);
    return SD_OK;
}

}  // namespace sd
