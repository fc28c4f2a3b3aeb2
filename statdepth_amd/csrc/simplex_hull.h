// simplex_hull.h -- device code the K4 kernels (simplex.hip) share with their retired generic generation
// (simplex_retired.hip, cross-check library only): the hull test from the data (point_in_hull), the enumeration and the
// sampling of the subsets, the block sum and the target selection, with the constants they need.  Everything here is
// inlined into the kernels of the two files.
#pragma once
#include "sd_common.h"
#include "point_select.h"

namespace sd {

constexpr int SMAX = 10;   // d + 1 <= 9
constexpr int SX_THREADS = 256;

__device__ static bool solve_subset(const double (*R)[SMAX + 1], int rank, const int *cols, double tol,
                                    double rank_eps) {
    double A[SMAX][SMAX + 1];
    for (int r = 0; r < rank; ++r) {
        for (int c = 0; c < rank; ++c) A[r][c] = R[r][cols[c]];
        A[r][rank] = R[r][SMAX];
    }
    for (int c = 0; c < rank; ++c) {
        int p = c;
        double best = fabs(A[c][c]);
        for (int r = c + 1; r < rank; ++r)
            if (fabs(A[r][c]) > best) { best = fabs(A[r][c]); p = r; }
        if (best <= rank_eps) return false;
        if (p != c)
            for (int k = 0; k <= rank; ++k) { double tmp = A[c][k]; A[c][k] = A[p][k]; A[p][k] = tmp; }
        for (int r = c + 1; r < rank; ++r) {
            double f = A[r][c] / A[c][c];
            for (int k = c; k <= rank; ++k) A[r][k] -= f * A[c][k];
        }
    }
    double l[SMAX];
    for (int c = rank - 1; c >= 0; --c) {
        double s = A[c][rank];
        for (int k = c + 1; k < rank; ++k) s -= A[c][k] * l[k];
        l[c] = s / A[c][c];
    }
    for (int c = 0; c < rank; ++c)
        if (!(l[c] >= -tol)) return false;
    return true;
}

// The system every site eliminates is NORMALISED: after the NaN / infinity checks the members and x are
// centred on the first member, and the coordinate rows, right-hand side included, are multiplied by 2^-e, e = ilogb of the
// largest centred |entry| of the MEMBERS (of x where they all coincide).  Both steps are exact for data that the subtraction
// does not round, so the decision is the same bit for bit under P -> 2^k P and under exact translations, and rank_eps and the
// consistency threshold are relative to the simplex's own extent.  An infinity that the subtraction or the scaling makes:
// outside.  The same statements, in the same order, as oracle_point_in_hull.
__device__ __forceinline__ bool sx_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for a NaN

// pts: kpts x d (row-major, local), x: d
__device__ static bool point_in_hull(const double *pts, int kpts, int d, const double *x, double tol) {
    int rows = d + 1;
    for (int c = 0; c < kpts * d; ++c)
        if (!sx_finite(pts[c])) return false;
    for (int r = 0; r < d; ++r)
        if (!sx_finite(x[r])) return false;
    double R[SMAX][SMAX + 1];
    double m = 0.0, mx = 0.0;                                    // the largest centred |entry| of the members, of x
    for (int r = 0; r < d; ++r) {
        for (int c = 0; c < kpts; ++c) {
            double v = pts[c * d + r] - pts[r];
            R[r][c] = v;
            if (fabs(v) > m) m = fabs(v);
        }
        double v = x[r] - pts[r];
        R[r][SMAX] = v;
        if (fabs(v) > mx) mx = fabs(v);
    }
    if (isinf(m) || isinf(mx)) return false;                     // the subtraction overflowed
    int e = m > 0.0 ? ilogb(m) : mx > 0.0 ? ilogb(mx) : 0;
    double scale = 1.0;
    for (int r = 0; r < d; ++r) {
        for (int c = 0; c < kpts; ++c) {
            R[r][c] = ldexp(R[r][c], -e);
            if (fabs(R[r][c]) > scale) scale = fabs(R[r][c]);
        }
        R[r][SMAX] = ldexp(R[r][SMAX], -e);
        if (fabs(R[r][SMAX]) > scale) scale = fabs(R[r][SMAX]);
    }
    for (int c = 0; c < kpts; ++c) R[d][c] = 1.0;
    R[d][SMAX] = 1.0;
    if (isinf(scale)) return false;                              // x that many extents away
    double rank_eps = 1e-10 * scale;
    int rank = 0;
    int lim = rows < kpts ? rows : kpts;
    for (; rank < lim; ++rank) {
        int pr = -1, pc = -1;
        double best = rank_eps;
        for (int r = rank; r < rows; ++r)
            for (int c = rank; c < kpts; ++c)
                if (fabs(R[r][c]) > best) { best = fabs(R[r][c]); pr = r; pc = c; }
        if (pr < 0) break;
        if (pr != rank)
            for (int k = 0; k <= SMAX; ++k) { double tmp = R[rank][k]; R[rank][k] = R[pr][k]; R[pr][k] = tmp; }
        if (pc != rank)
            for (int r = 0; r < rows; ++r) { double tmp = R[r][rank]; R[r][rank] = R[r][pc]; R[r][pc] = tmp; }
        for (int r = rank + 1; r < rows; ++r) {
            double f = R[r][rank] / R[rank][rank];
            if (f != 0.0) {
                for (int c = rank; c < kpts; ++c) R[r][c] -= f * R[rank][c];
                R[r][SMAX] -= f * R[rank][SMAX];
            }
        }
    }
    for (int r = rank; r < rows; ++r)
        if (fabs(R[r][SMAX]) > 1e-7 * scale) return false;
    int cols[SMAX];
    for (int c = 0; c < rank; ++c) cols[c] = c;
    if (rank == kpts) return solve_subset(R, rank, cols, tol, rank_eps);
    for (;;) {
        if (solve_subset(R, rank, cols, tol, rank_eps)) return true;
        int k = rank - 1;
        while (k >= 0 && cols[k] == kpts - rank + k) --k;
        if (k < 0) break;
        ++cols[k];
        for (int l = k + 1; l < rank; ++l) cols[l] = cols[l - 1] + 1;
    }
    return false;
}

__device__ static u64 binom_dev(u64 a, int k) {
    if (k < 0 || (u64)k > a) return 0;
    u64 c = 1;
    for (int j = 1; j <= k; ++j) c = c * (a - (u64)j + 1) / (u64)j;
    return c;
}

// lexicographic unranking of the r-th k-subset of {0..no-1}
__device__ static void unrank_comb(u64 r, int k, i64 no, i64 *idx) {
    i64 c = 0;
    for (int p = 0; p < k; ++p) {
        for (;; ++c) {
            u64 cnt = binom_dev((u64)(no - 1 - c), k - 1 - p);   // subsets starting with c at position p
            if (r < cnt) break;
            r -= cnt;
        }
        idx[p] = c++;
    }
}

__device__ static bool next_comb(i64 *idx, int k, i64 no) {
    int i = k - 1;
    while (i >= 0 && idx[i] == no - k + i) --i;
    if (i < 0) return false;
    ++idx[i];
    for (int l = i + 1; l < k; ++l) idx[l] = idx[l - 1] + 1;
    return true;
}

// splitmix64 finaliser: counter-based draws keyed by (seed, target, sample, draw)
__device__ __host__ static inline u64 mix64(u64 z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The sampled estimators' subsets (round 4): shared sample s is ONE (d+1)-subset of all n rows for every target -- k distinct rows
// drawn with the counter generator keyed by (seed, s): index = floor(r * n / 2^64), rejection on duplicates, sorted ascending -- so
// that its factorisation can be shared by all targets (sxw_factor_kernel / sxw_apply_kernel).  A target uses the FIRST `samples`
// shared subsets that do not contain it (s = 0, 1, 2, ... in order): each is uniform over the subsets of the other rows.
// Restated identically in oracle.c (sample_rows / oracle_simplex_sampled).
constexpr u64 SX_SHARED_KEY = 0xFFFFFFFFFFFFFFFFull;
__device__ static void sample_rows(u64 seed, u64 keyv, u64 sample, int k, i64 n, i64 *idx) {
    u64 key = mix64(seed ^ mix64(keyv * 0xD1342543DE82EF95ull + sample));
    u64 ctr = 0;
    for (int p = 0; p < k;) {
        u64 r = mix64(key + ctr++);
        // index in [0, n) as the high half of r * n (a 64 x 64 -> 128 bit product: a handful of instructions; the 64-bit
        // modulo it replaces was ~480 of the 715 lane-instructions of a sampled 4-point test, profiles/r02_issue_roofline.json)
        i64 c = (i64)__umul64hi(r, (u64)n);
        bool dup = false;
        for (int l = 0; l < p; ++l) dup |= (idx[l] == c);
        if (!dup) idx[p++] = c;
    }
    for (int a = 1; a < k; ++a) {   // insertion sort
        i64 v = idx[a];
        int b = a - 1;
        while (b >= 0 && idx[b] > v) { idx[b + 1] = idx[b]; --b; }
        idx[b + 1] = v;
    }
}
// the next shared subset from index *s on that does not contain row tg; *s is left behind it
__device__ static void sample_next_valid(u64 seed, i64 tg, u64 *s, int k, i64 n, i64 *idx) {
    for (;;) {
        sample_rows(seed, SX_SHARED_KEY, (*s)++, k, n, idx);
        bool member = false;
        for (int l = 0; l < k; ++l) member |= idx[l] == tg;
        if (!member) return;
    }
}

__device__ __forceinline__ u64 block_sum_u64(u64 v, u64 *scratch) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 r = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < SX_THREADS / 64; ++k) r += scratch[k];
    return r;
}

// The targets are selected by a PointSel (point_select.h); the subsets are drawn from a target's others.  The external
// and the block form are for point clouds only (T = 0); a block is enumerated exhaustively whatever `total` says.
__device__ __forceinline__ u64 sx_total(const PointView &v, int k, u64 total) {
    return v.mem ? binom_dev((u64)v.others(), k) : total;
}

// row of P behind index i of a subset.  direct (sx_direct, taken once per thread): i is a row already
__device__ __forceinline__ bool sx_direct(const PointView &v, i64 samples) {
    return samples >= 0 || v.tg < 0;                             // a sampled subset holds rows, never the target's; no row to skip
}
__device__ __forceinline__ i64 sx_src(const PointView &v, bool direct, i64 i) {
    if (v.mem) return v.mem[i];
    if (direct) return i;
    return i < v.tg ? i : i + 1;                                 // skip the target itself
}

}  // namespace sd
