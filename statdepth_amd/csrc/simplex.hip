// simplex.hip -- K4: batched point-in-simplex containment counts.
//
// Replaces _is_in_simplex (_containment.py:138-176; an LP feasibility problem handed
// to scipy.optimize.linprog: sum l_k p_k = x, sum l_k = 1, l >= 0) inside the subset
// loops of _pointwisedepth (_pointcloud.py:50-54) and _simplex_depth /
// _simplex_containment (_functional.py:281-285, _containment.py:130-136).
//
// point_in_hull() is the same restatement as oracle_point_in_hull (oracle/oracle.c):
// complete-pivoting elimination of [P^T;1] l = [x;1]; full rank -> unique l, inside
// iff min l >= -tol; rank deficient (degenerate simplex) -> enumerate `rank`-subsets
// (Caratheodory).  Same operation order as the oracle so decisions agree bit for bit
// (this file is compiled with -ffp-contract=off).
//
// Work decomposition: threads own contiguous ranges of the lexicographic subset
// enumeration (unrank once, then step), or one sampled subset each in the sampled
// estimators.  Small dense fp64 systems per thread: VALU bound, no MFMA (systems are
// (d+1)x(d+1) with d <= 8 and data-dependent pivoting).
//
// The device code below the register-resident forms -- point_in_hull, the enumeration, the sampling -- is in simplex_hull.h,
// shared with the generic scratch-memory generation (simplex_retired.hip, cross-check library only).  Which kernels a call
// runs is stated once, at SxwPlan.
#include <stdlib.h>

#include "simplex_hull.h"

namespace sd {

// The loaders of the register-resident forms.  sx_members: columns 0 .. D of R from the members row(0) .. row(D), centred on
// row(0) (kept in p0) and scaled by 2^-e; `scale` = the scaled member maximum, in [1, 2), or 1 where all members coincide
// (then e = 0: the system is rank deficient and point_in_hull decides it from the data).  False: a NaN or an infinity.
// sx_target: the last column of R from x with the same p0 and e, `scale` raised to its largest |entry|; an infinity there
// is hull_full_rank's to refuse.  e depends on the members alone, which keeps the shared factorisation replayable.
template <int D, int W, typename Row>
__device__ __forceinline__ bool sx_members(double (&R)[D + 1][W], Row row, double (&p0)[D], int &e, double &scale) {
    bool ok = true;
    double m = 0.0;
    const double *q0 = row(0);
#pragma unroll
    for (int r = 0; r < D; ++r) p0[r] = q0[r];
#pragma unroll
    for (int c = 0; c <= D; ++c) {
        const double *pp = row(c);
#pragma unroll
        for (int r = 0; r < D; ++r) {
            const double v = pp[r];
            ok &= sx_finite(v);
            const double w = v - p0[r];
            R[r][c] = w;
            m = fabs(w) > m ? fabs(w) : m;
        }
        R[D][c] = 1.0;
    }
    ok = ok && sx_finite(m);
    e = ok && m > 0.0 ? ilogb(m) : 0;
#pragma unroll
    for (int c = 0; c <= D; ++c)
#pragma unroll
        for (int r = 0; r < D; ++r) R[r][c] = ldexp(R[r][c], -e);
    const double ms = ldexp(m, -e);                                     // exact and monotone: the maximum of the scaled entries
    scale = ms > 1.0 ? ms : 1.0;
    return ok;
}

template <int D, int W>
__device__ __forceinline__ bool sx_target(double (&R)[D + 1][W], const double *xx, const double (&p0)[D], int e, double &scale) {
    bool ok = true;
#pragma unroll
    for (int r = 0; r < D; ++r) {
        const double v = xx[r];
        ok &= sx_finite(v);
        const double w = ldexp(v - p0[r], -e);
        R[r][W - 1] = w;
        scale = fabs(w) > scale ? fabs(w) : scale;
    }
    R[D][W - 1] = 1.0;
    return ok;
}

// ---------------------------------------------------------------------------------------------------
// Register-resident form of the same test for a compile-time dimension D and a NON-degenerate simplex
// (D + 1 points of full rank -- every simplex of continuous data).  The (D+1) x (D+2) system lives in VGPRs:
// every array index below is a compile-time constant, and the data-dependent row / column exchanges of the
// pivoting are predicated exchanges with each candidate (v_cndmask) instead of indexed moves through scratch
// memory.  The arithmetic is, operation for operation and in the same order, that of point_in_hull() /
// solve_subset() above (pivot search order and strict ">" included), so the decision is the same bit for bit.
// Returns 0 / 1 (outside / inside) or 2: the simplex is rank deficient, the caller falls back to point_in_hull().
// ---------------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ int hull_full_rank(double (&R)[D + 1][D + 2], double scale, double tol) {
    constexpr int K = D + 1;                  // points = rows = K; column K is the right-hand side
    if (isinf(scale)) return 0;
    const double rank_eps = 1e-10 * scale;
    // ---- complete-pivoting elimination (point_in_hull) ----
#pragma unroll
    for (int rank = 0; rank < K; ++rank) {
        int pr = -1, pc = -1;
        double best = rank_eps;
#pragma unroll
        for (int r = rank; r < K; ++r)
#pragma unroll
            for (int c = rank; c < K; ++c) {
                const double a = fabs(R[r][c]);
                const bool gt = a > best;
                best = gt ? a : best;
                pr = gt ? r : pr;
                pc = gt ? c : pc;
            }
        if (pr < 0) return 2;                 // rank deficient: Caratheodory enumeration in the generic code
#pragma unroll
        for (int rr = rank + 1; rr < K; ++rr) {           // exchange rows rank <-> pr
            const bool sw = pr == rr;
#pragma unroll
            for (int k = 0; k <= K; ++k) {
                const double a = R[rank][k], b = R[rr][k];
                R[rank][k] = sw ? b : a;
                R[rr][k] = sw ? a : b;
            }
        }
#pragma unroll
        for (int cc = rank + 1; cc < K; ++cc) {           // exchange columns rank <-> pc
            const bool sw = pc == cc;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const double a = R[r][rank], b = R[r][cc];
                R[r][rank] = sw ? b : a;
                R[r][cc] = sw ? a : b;
            }
        }
#pragma unroll
        for (int r = rank + 1; r < K; ++r) {
            const double f = R[r][rank] / R[rank][rank];
            const bool nz = f != 0.0;
#pragma unroll
            for (int c = rank; c <= K; ++c) {
                const double v = R[r][c] - f * R[rank][c];
                R[r][c] = nz ? v : R[r][c];
            }
        }
    }
    // ---- solve_subset with all K columns: partial pivoting on the (already triangular) system ----
#pragma unroll
    for (int c = 0; c < K; ++c) {
        int p = c;
        double best = fabs(R[c][c]);
#pragma unroll
        for (int r = c + 1; r < K; ++r) {
            const double a = fabs(R[r][c]);
            const bool gt = a > best;
            best = gt ? a : best;
            p = gt ? r : p;
        }
        if (best <= rank_eps) return 0;
#pragma unroll
        for (int rr = c + 1; rr < K; ++rr) {
            const bool sw = p == rr;
#pragma unroll
            for (int k = 0; k <= K; ++k) {
                const double a = R[c][k], b = R[rr][k];
                R[c][k] = sw ? b : a;
                R[rr][k] = sw ? a : b;
            }
        }
#pragma unroll
        for (int r = c + 1; r < K; ++r) {
            const double f = R[r][c] / R[c][c];
#pragma unroll
            for (int k = c; k <= K; ++k) R[r][k] -= f * R[c][k];
        }
    }
    double l[K];
#pragma unroll
    for (int c = K - 1; c >= 0; --c) {
        double sacc = R[c][K];
#pragma unroll
        for (int k = c + 1; k < K; ++k) sacc -= R[c][k] * l[k];
        l[c] = sacc / R[c][c];
    }
    bool in = true;
#pragma unroll
    for (int c = 0; c < K; ++c) in = in && (l[c] >= -tol);
    return in ? 1 : 0;
}

// grid = (chunks, m), the work decomposition of the generic kernel (simplex_retired.hip); D = d known at compile time.
template <int D>
__global__ __launch_bounds__(SX_THREADS) void simplex_kernel_fast(
    const double *__restrict__ P, i64 n, i64 T, PointSel sel, int relax, double tol,
    u64 total, u64 per_thread, i64 samples, u64 seed, i64 q0, u64 *__restrict__ out) {
    __shared__ u64 scratch[SX_THREADS / 64];
    constexpr int K = D + 1;
    const i64 q = q0 + blockIdx.y;
    const PointView blk = point_view(sel, P, n, D, q);
    const i64 tg = blk.tg, no = blk.others();
    const bool direct = sx_direct(blk, samples);
    total = sx_total(blk, K, total);
    const u64 tid = (u64)blockIdx.x * SX_THREADS + threadIdx.x;
    const u64 first = tid * per_thread;
    u64 acc = 0;
    if (first < total) {
        const u64 last = first + per_thread < total ? first + per_thread : total;
        i64 idx[SMAX];
        if (samples < 0) unrank_comb(first, K, no, idx);
        u64 snext = 0;                                                  // sampled: the shared index behind the last subset taken
        if (samples >= 0)
            for (u64 r = 0; r < first; ++r) sample_next_valid(seed, tg, &snext, K, n, idx);   // this thread's first valid subset
        const i64 TT = T > 0 ? T : 1;
        for (u64 r = first; r < last; ++r) {
            if (samples >= 0) sample_next_valid(seed, tg, &snext, K, n, idx);
            u64 cnt = 0;
            for (i64 t = 0; t < TT; ++t) {
                double R[K][K + 1], p0[D];
                double scale;
                int e;
                const double *xx = T > 0 ? P + (tg * TT + t) * D : blk.x;  // curves (rows form only): the target at timepoint t
                bool ok = sx_members<D>(R, [&](int c) { return P + (sx_src(blk, direct, idx[c]) * TT + t) * D; }, p0, e, scale);
                ok &= sx_target<D>(R, xx, p0, e, scale);
                int res = ok ? hull_full_rank<D>(R, scale, tol) : 0;
                if (res == 2) {                                         // degenerate simplex: generic code, from the data
                    double pts[SMAX * 8], x[8];
                    for (int c = 0; c < K; ++c) {
                        const i64 src = sx_src(blk, direct, idx[c]);
                        const double *pp = P + (src * TT + t) * D;
                        for (int e = 0; e < D; ++e) pts[c * D + e] = pp[e];
                    }
                    for (int e = 0; e < D; ++e) x[e] = xx[e];
                    res = point_in_hull(pts, K, D, x, tol) ? 1 : 0;
                }
                cnt += (u64)res;
            }
            acc += (T > 0 && !relax) ? (cnt / (u64)TT) : cnt;
            if (samples < 0 && r + 1 < last) next_comb(idx, K, no);
        }
    }
    u64 tot = block_sum_u64(acc, scratch);
    if (threadIdx.x == 0 && tot) atomicAdd(&out[q], tot);
}


// ---------------------------------------------------------------------------------------------------
// Sampled estimators, every target's sample s the SAME subset (sample_rows above): the subset's matrix [P_S^T; 1] is
// eliminated ONCE and every target only carries its right-hand side [x; 1] through the recorded row operations.
// point_in_hull() / solve_subset() touch the right-hand side in a fixed sequence of operations that depends on the matrix
// alone -- the row exchanges of the complete-pivoting elimination, b_r -= f b_k for its multipliers f (skipped where f = 0),
// the second (partial-pivoting) elimination of solve_subset on the triangular system with its own multipliers, the back
// substitution -- so replaying that sequence gives the barycentric coordinates of the per-target elimination BIT FOR BIT,
// at about 2 K^2 multiply-subtracts + K divisions per test instead of a K x K elimination (d = 8: ~400 instructions
// against ~7 500; d = 3: ~90 against ~700, and no random gathers: the members are read once per subset).
// The system is the normalised one (above): the record carries the subset's first member p0 (in final row order) and its exponent e,
// functions of the subset alone, and a target's right-hand side for this subset is 2^-e (x - p0).
// What depends on the target besides the right-hand side is `scale` (it includes that |x|) through rank_eps = 1e-10 scale: a
// target whose own scale would put the smallest pivot at or below rank_eps, and a subset that is rank deficient, holds a NaN
// or an infinity, or exchanges rows in the second elimination, take the per-target code (point_in_hull), decision for decision
// the old kernel's.  A target that is a MEMBER of the subset skips it and takes a spare shared subset instead (the first
// `samples` shared subsets that do not contain it: sxw_members_kernel counts what it skips, sxw_spare_kernel makes it up).
// Two kernels over a caller's workspace (SxwPlan): the records go to HBM, a thread per (timepoint, sample) with the whole
// register file for its elimination, and the replay reads a record as one coalesced load per wave, in batches of pairs as
// large as the workspace holds.
// ---------------------------------------------------------------------------------------------------
// the per-target code for a target the shared replay cannot serve (see above): out of line, so that its scratch arrays and
// registers are not the replay loop's
template <int D>
__device__ __noinline__ int sxw_special(const double *P, i64 TT, i64 t, const int *mem, const double *xv, double tol) {
    constexpr int K = D + 1;
    double pts[SMAX * 8], x[8];
    for (int c = 0; c < K; ++c) {
        const double *pp = P + ((i64)mem[c] * TT + t) * D;
        for (int e = 0; e < D; ++e) pts[c * D + e] = pp[e];
    }
    for (int e = 0; e < D; ++e) x[e] = xv[e];
    return point_in_hull(pts, K, D, x, tol) ? 1 : 0;
}

template <int D> struct SxwCfg {
    static constexpr int K = D + 1, NL = K * (K - 1) / 2, NU = K * (K + 1) / 2;
    static constexpr int DW = 2 * NL + NU + 2 + K;                      // doubles: f1, f2, u, scale, minpiv, p0 (the first member) by final row
    static constexpr int IW = ((2 * K + 2 + 3) / 4) * 4;                // ints: perm, members, status, e; padded to 16 bytes
    static constexpr size_t REC = (size_t)DW * 8 + (size_t)IW * 4;      // bytes of a record
    static constexpr int TPT = D >= 5 ? 2 : 4;                          // targets per thread of the replay
};

// pairs [w0, w0 + cnt) of the call, pair w = timepoint w / samples, sample w % samples; one thread each
template <int D>
__global__ __launch_bounds__(64) void sxw_factor_kernel(const double *__restrict__ P, i64 n, i64 T, i64 samples, u64 seed, i64 w0, i64 cnt,
                                                        double *__restrict__ recd, int *__restrict__ reci, double *__restrict__ m1g) {
    using C = SxwCfg<D>;
    constexpr int K = C::K, NL = C::NL, NU = C::NU, DW = C::DW, IW = C::IW;
    const i64 v = (i64)blockIdx.x * 64 + threadIdx.x;
    if (v >= cnt) return;
    const i64 TT = T > 0 ? T : 1;
    const i64 t = (w0 + v) / samples, sidx = (w0 + v) % samples;
    i64 idx[K];
    sample_rows(seed, SX_SHARED_KEY, (u64)sidx, K, n, idx);
    double *rd = recd + (size_t)v * DW;
    int *ri = reci + (size_t)v * IW;
    double *m1l = m1g + (size_t)v * (K * (K - 1));                      // the first elimination's multipliers by ORIGINAL row
    double R[K][K], p0[D];
    int rowid[K];
    double scale;
    int e;
    // the normalised matrix: p0, e and scale are functions of the subset alone
    bool irregular = !sx_members<D>(R, [&](int c) { return P + (idx[c] * TT + t) * D; }, p0, e, scale);
#pragma unroll
    for (int i = 0; i < K; ++i) rowid[i] = i;
    const double rank_eps = 1e-10 * scale;
    double minpiv = __builtin_huge_val();
#pragma unroll
    for (int rank = 0; rank < K; ++rank) {
        int pr = -1, pc = -1;
        double best = rank_eps;
#pragma unroll
        for (int r = rank; r < K; ++r)
#pragma unroll
            for (int c = rank; c < K; ++c) {
                const double av = fabs(R[r][c]);
                const bool gt = av > best;
                best = gt ? av : best;
                pr = gt ? r : pr;
                pc = gt ? c : pc;
            }
        irregular |= pr < 0;                                            // rank deficient: the per-target code's business
        minpiv = best < minpiv ? best : minpiv;
#pragma unroll
        for (int rr = rank + 1; rr < K; ++rr) {                         // exchange rows rank <-> pr
            const bool sw = pr == rr;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double x0 = R[rank][k], x1 = R[rr][k];
                R[rank][k] = sw ? x1 : x0;
                R[rr][k] = sw ? x0 : x1;
            }
            const int i0 = rowid[rank], i1 = rowid[rr];
            rowid[rank] = sw ? i1 : i0;
            rowid[rr] = sw ? i0 : i1;
        }
#pragma unroll
        for (int cc = rank + 1; cc < K; ++cc) {                         // exchange columns rank <-> pc
            const bool sw = pc == cc;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const double x0 = R[r][rank], x1 = R[r][cc];
                R[r][rank] = sw ? x1 : x0;
                R[r][cc] = sw ? x0 : x1;
            }
        }
#pragma unroll
        for (int r = rank + 1; r < K; ++r) {
            const double f = R[r][rank] / R[rank][rank];
            if (rank < K - 1) m1l[rowid[r] * (K - 1) + rank] = f;
            const bool nz = f != 0.0;
#pragma unroll
            for (int c = rank; c < K; ++c) {
                const double x = R[r][c] - f * R[rank][c];
                R[r][c] = nz ? x : R[r][c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const double best = fabs(R[c][c]);
#pragma unroll
        for (int r = c + 1; r < K; ++r) irregular |= fabs(R[r][c]) > best;
        minpiv = best < minpiv ? best : minpiv;
#pragma unroll
        for (int r = c + 1; r < K; ++r) {
            const double f = R[r][c] / R[c][c];
            rd[NL + r * (r - 1) / 2 + c] = f;
#pragma unroll
            for (int k = c; k < K; ++k) R[r][k] -= f * R[c][k];
        }
    }
    __threadfence_block();                                              // this thread's own multipliers, read back by row below
#pragma unroll
    for (int i = 1; i < K; ++i)
#pragma unroll
        for (int k = 0; k < i; ++k) rd[i * (i - 1) / 2 + k] = m1l[rowid[i] * (K - 1) + k];
    {
        int w = 0;
#pragma unroll
        for (int c = 0; c < K; ++c)
#pragma unroll
            for (int k = c; k < K; ++k) rd[2 * NL + w++] = R[c][k];
    }
    rd[2 * NL + NU] = scale;
    rd[2 * NL + NU + 1] = minpiv;
#pragma unroll
    for (int i = 0; i < K; ++i) {                                       // p0 in the final row order (the row of ones: 0), as the replay gathers b
        double v = 0.0;
#pragma unroll
        for (int r = 0; r < D; ++r) v = rowid[i] == r ? p0[r] : v;
        rd[2 * NL + NU + 2 + i] = v;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) { ri[i] = rowid[i]; ri[K + i] = (int)idx[i]; }
    ri[2 * K] = irregular ? 1 : 0;
    ri[2 * K + 1] = e;
}

// replay of pairs [w0, w0 + cnt) on a tile of targets: grid = (tiles, splits); counts leave as one atomic per target
template <int D>
__global__ __launch_bounds__(256) void sxw_apply_kernel(const double *__restrict__ P, i64 n, i64 T, const i64 *__restrict__ targets, i64 m,
                                                       double tol, i64 samples, u64 seed, i64 w0, i64 cnt,
                                                       const double *__restrict__ recd, const int *__restrict__ reci,
                                                       u64 *__restrict__ out) {
    using C = SxwCfg<D>;
    constexpr int K = C::K, NL = C::NL, NU = C::NU, DW = C::DW, IW = C::IW, TPT = C::TPT;
    const int tid = threadIdx.x;
    const i64 TT = T > 0 ? T : 1;
    const i64 q0 = (i64)blockIdx.x * (256 * TPT);
    i64 tg[TPT];
    bool live[TPT];
    u64 acc[TPT];
#pragma unroll
    for (int p = 0; p < TPT; ++p) {
        const i64 q = q0 + tid + (i64)p * 256;
        live[p] = q < m;
        tg[p] = live[p] ? (targets ? targets[q] : q) : 0;
        acc[p] = 0;
    }
    // this workgroup's slice of the batch: contiguous (the timepoint changes rarely)
    const i64 per = (cnt + gridDim.y - 1) / gridDim.y;
    const i64 vbeg = (i64)blockIdx.y * per, vend = vbeg + per < cnt ? vbeg + per : cnt;
    i64 tcur = -1;
    double xx[TPT][K];
    bool xnan[TPT];
    // A record travels as ONE coalesced load per wave (lane L holds doubles L and 64 + L, and int L), prefetched a pair ahead;
    // its values reach the arithmetic through v_readlane with compile-time lane numbers: wave-uniform operands in SGPRs without
    // the scalar cache's latency per value (a scalar load per value, waited for one by one, was ten times slower) and without LDS.
    static_assert(DW <= 128 && IW <= 64, "a record fits two doubles and one int per lane");
    const int lane = tid & 63;
    double c0 = 0.0, c1 = 0.0, n0 = 0.0, n1 = 0.0;
    int ci = 0, ni = 0;
    auto fetch = [&](i64 v, double &d0, double &d1, int &di) {
        const double *rd = recd + (size_t)v * DW;
        d0 = lane < DW ? rd[lane] : 0.0;
        d1 = 64 + lane < DW ? rd[64 + lane] : 0.0;
        di = lane < IW ? reci[(size_t)v * IW + lane] : 0;
    };
    if (vbeg < vend) fetch(vbeg, n0, n1, ni);
#pragma unroll 1
    for (i64 v = vbeg; v < vend; ++v) {
        c0 = n0; c1 = n1; ci = ni;
        if (v + 1 < vend) fetch(v + 1, n0, n1, ni);
        auto RD = [&](int k) -> double {                                // k: a compile-time constant wherever this is called
            const unsigned long long bits = (unsigned long long)__double_as_longlong(k < 64 ? c0 : c1);
            const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)bits, k & 63);
            const u32 hi = (u32)__builtin_amdgcn_readlane((int)(u32)(bits >> 32), k & 63);
            return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        };
        auto RI = [&](int k) -> int { return __builtin_amdgcn_readlane(ci, k); };
        const i64 t = (w0 + v) / samples;
        if (t != tcur) {                                                // block-uniform
            tcur = t;
#pragma unroll
            for (int p = 0; p < TPT; ++p) {
                const double *xp = P + (tg[p] * TT + t) * D;
                xnan[p] = false;
#pragma unroll
                for (int e = 0; e < D; ++e) { xx[p][e] = xp[e]; xnan[p] |= xp[e] != xp[e]; }
                xx[p][D] = 1.0;
            }
        }
        const double scaleS = RD(2 * NL + NU), minpiv = RD(2 * NL + NU + 1);
        const int status = RI(2 * K);
        int perm[K], mem[K];
#pragma unroll
        for (int i = 0; i < K; ++i) { perm[i] = RI(i); mem[i] = RI(K + i); }
        const int ex = RI(2 * K + 1);
        bool special[TPT], in[TPT], skip[TPT];
        double b[TPT][K], l[TPT][K], sc[TPT];
#pragma unroll
        for (int p = 0; p < TPT; ++p) {
            bool member = false;
#pragma unroll
            for (int i = 0; i < K; ++i) member |= (i64)mem[i] == tg[p];
            skip[p] = member;                                           // this target takes a spare subset instead (sxw_spare_kernel)
            in[p] = true;
            sc[p] = scaleS;
        }
        // the right-hand side of this subset's normalised system, in its final row order: x centred on the subset's first member
        // and scaled by its 2^-e; the row of ones (p0 = 0 there, and no scaling) stays 1.  Unconditional arithmetic: no branches.
#pragma unroll
        for (int p = 0; p < TPT; ++p)
#pragma unroll
            for (int i = 0; i < K; ++i) b[p][i] = xx[p][perm[i]];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const double p0i = RD(2 * NL + NU + 2 + i);
            const int exi = perm[i] == D ? 0 : -ex;                      // block-uniform
#pragma unroll
            for (int p = 0; p < TPT; ++p) {
                const double w = ldexp(b[p][i] - p0i, exi);
                b[p][i] = w;
                sc[p] = fmax(sc[p], fabs(w));                           // w is a NaN only where x is: xnan
            }
        }
        // a NaN, or an infinity in x or made by the subtraction or the scaling: the per-target code says no
#pragma unroll
        for (int p = 0; p < TPT; ++p) special[p] = status != 0 || xnan[p] || !(minpiv > 1e-10 * sc[p]) || isinf(sc[p]);
        if (status == 0) {                                              // block-uniform
            int w = 0;
#pragma unroll
            for (int i = 1; i < K; ++i)
#pragma unroll
                for (int k = 0; k < i; ++k) {
                    const double f = RD(w++);
                    if (f != 0.0) {                                     // block-uniform
#pragma unroll
                        for (int p = 0; p < TPT; ++p) b[p][i] -= f * b[p][k];
                    }
                }
            w = 0;
#pragma unroll
            for (int i = 1; i < K; ++i)
#pragma unroll
                for (int k = 0; k < i; ++k) {
                    const double f = RD(NL + w++);
#pragma unroll
                    for (int p = 0; p < TPT; ++p) b[p][i] -= f * b[p][k];
                }
#pragma unroll
            for (int c = K - 1; c >= 0; --c) {
                const int base = 2 * NL + c * K - c * (c - 1) / 2;      // u[c][c]
                double sacc[TPT];
#pragma unroll
                for (int p = 0; p < TPT; ++p) sacc[p] = b[p][c];
#pragma unroll
                for (int k = c + 1; k < K; ++k) {
                    const double u = RD(base + (k - c));
#pragma unroll
                    for (int p = 0; p < TPT; ++p) sacc[p] -= u * l[p][k];
                }
                const double dg = RD(base);
#pragma unroll
                for (int p = 0; p < TPT; ++p) {
                    l[p][c] = sacc[p] / dg;
                    in[p] = in[p] && (l[p][c] >= -tol);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < TPT; ++p) {
            if (!live[p] || skip[p]) continue;
            int inside = in[p] ? 1 : 0;
            if (special[p]) {
                double xv[D];
#pragma unroll
                for (int e = 0; e < D; ++e) xv[e] = xx[p][e];
                inside = sxw_special<D>(P, TT, t, mem, xv, tol);
            }
            acc[p] += (u64)inside;
        }
    }
#pragma unroll
    for (int p = 0; p < TPT; ++p)
        if (live[p] && acc[p]) atomicAdd(&out[q0 + tid + (i64)p * 256], acc[p]);
}

// cmem[row] = shared subsets s < samples that contain the row: what a target of that row skips in the replay
__global__ __launch_bounds__(256) void sxw_members_kernel(i64 n, i64 samples, u64 seed, int k, int *__restrict__ cmem) {
    const i64 sidx = (i64)blockIdx.x * 256 + threadIdx.x;
    if (sidx >= samples) return;
    i64 idx[SMAX];
    sample_rows(seed, SX_SHARED_KEY, (u64)sidx, k, n, idx);
    for (int i = 0; i < k; ++i) atomicAdd(&cmem[idx[i]], 1);
}

// the spare subsets of the targets that skipped some: a thread per (target, timepoint) walks the shared subsets from index
// `samples` on, takes those that do not contain its target until it has made up what it skipped, and tests each with the
// per-target code (hull_full_rank, point_in_hull for a degenerate simplex).  K / n of the tests go this way.
template <int D>
__global__ __launch_bounds__(256) void sxw_spare_kernel(const double *__restrict__ P, i64 n, i64 T, const i64 *__restrict__ targets, i64 m,
                                                       double tol, i64 samples, u64 seed, const int *__restrict__ cmem,
                                                       u64 *__restrict__ out) {
    constexpr int K = D + 1;
    const i64 TT = T > 0 ? T : 1;
    const i64 id = (i64)blockIdx.x * 256 + threadIdx.x;
    if (id >= m * TT) return;
    const i64 q = id / TT, t = id % TT;
    const i64 tg = targets ? targets[q] : q;
    const int need = cmem[tg];
    if (need == 0) return;
    u64 snext = (u64)samples, acc = 0;
    const double *xx = P + (tg * TT + t) * D;
    for (int got = 0; got < need; ++got) {
        i64 idx[K];
        sample_next_valid(seed, tg, &snext, K, n, idx);
        double R[K][K + 1], p0[D];
        double scale;
        int e;
        bool ok = sx_members<D>(R, [&](int c) { return P + (idx[c] * TT + t) * D; }, p0, e, scale);
        ok &= sx_target<D>(R, xx, p0, e, scale);
        int res = ok ? hull_full_rank<D>(R, scale, tol) : 0;
        if (res == 2) {                                                 // degenerate simplex: generic code, from the data
            double pts[SMAX * 8], x[8];
            for (int c = 0; c < K; ++c) {
                const double *pp = P + (idx[c] * TT + t) * D;
                for (int e = 0; e < D; ++e) pts[c * D + e] = pp[e];
            }
            for (int e = 0; e < D; ++e) x[e] = xx[e];
            res = point_in_hull(pts, K, D, x, tol) ? 1 : 0;
        }
        acc += (u64)res;
    }
    if (acc) atomicAdd(&out[q], acc);
}

// ---------------------------------------------------------------------------------------------------
// The routes of a call, and the workspace of the one that needs it.
//   per target  simplex_kernel_fast<D>, a thread per range of subsets: every exhaustive call, and the sampled ones that the
//               replay does not serve -- external targets, blocks, relax = False, n < d + 3, or a workspace below the floor
//               (none: ws null).  Same subsets as the replay, so the counts are the same.
//   replay      sampled, targets of the set, counts that add over the timepoints (point clouds, relax = True), n >= d + 3
//               and ws_bytes >= floor: sxw_members_kernel, per batch of pairs sxw_factor_kernel + sxw_apply_kernel,
//               sxw_spare_kernel.
//   Cross-check library only: SD_SIMPLEX_PERTARGET = 1 keeps a call off the replay, SD_SIMPLEX_GENERIC = 1 runs the per-target
//   route on the retired generic kernel (retired_simplex_generic).
// The workspace behind its base rounded up to ALIGN: the member counts (an int per row), then a batch's records (recd,
// reci) and first-elimination multipliers (m1g), `per` bytes a pair.  The recommended size holds every pair of the call up
// to MAX_BATCH (~1.7 GB at d = 8); the floor is that of FLOOR_SAMPLES samples, a few hundred records.
// ---------------------------------------------------------------------------------------------------
struct SxwPlan {
    static constexpr size_t ALIGN = 256, CARVE_SLACK = 768, SIZE_SLACK = 1024;   // set aside by the carve (the base's rounding); by the sizes
    static constexpr i64 MAX_BATCH = (i64)1 << 20, FLOOR_SAMPLES = 256;
    size_t per, cm_bytes;                                               // bytes per pair; of the member counts
    size_t bytes, floor;                                                // recommended; the least the replay is taken with
    i64 pairs, batch;                                                   // (timepoint, sample) pairs of the call; per round, 0: below the floor
    size_t cmem, recd, m1g, reci;                                       // offsets behind the rounded base, for `batch` pairs
};
// ws_bytes: what is at hand (0: the sizes alone).  d outside [1, 8] or samples <= 0: all zero
static SxwPlan sxw_plan(i64 n, i64 T, int d, i64 samples, size_t ws_bytes) {
    SxwPlan p = {};
    if (d < 1 || d > 8 || samples <= 0) return p;
    size_t dw = 0;                                                      // bytes of a record's doubles
    SD_DISPATCH_D(d, p.per = SxwCfg<D_>::REC + (size_t)(D_ + 1) * D_ * 8; dw = (size_t)SxwCfg<D_>::DW * 8)
    const i64 TT = T > 0 ? T : 1;
    p.pairs = samples * TT;
    p.cm_bytes = align_up((size_t)n * 4, SxwPlan::ALIGN);
    auto size_of = [&](i64 pairs) {
        return (size_t)(pairs < SxwPlan::MAX_BATCH ? pairs : SxwPlan::MAX_BATCH) * p.per + p.cm_bytes + SxwPlan::SIZE_SLACK;
    };
    p.bytes = size_of(p.pairs);
    p.floor = size_of((samples < SxwPlan::FLOOR_SAMPLES ? samples : SxwPlan::FLOOR_SAMPLES) * TT);
    if (ws_bytes < p.floor) return p;
    p.batch = (i64)((ws_bytes - SxwPlan::CARVE_SLACK - p.cm_bytes) / p.per);
    if (p.batch > p.pairs) p.batch = p.pairs;
    p.recd = p.cmem + p.cm_bytes;
    p.m1g = p.recd + (size_t)p.batch * dw;
    p.reci = p.m1g + (size_t)p.batch * (size_t)((d + 1) * d) * 8;
    return p;
}

size_t simplex_sampled_workspace_bytes(i64 n, i64 T, int d, i64 samples) { return sxw_plan(n, T, d, samples, 0).bytes; }

template <int D>
static int launch_simplex_ws(const double *P, i64 n, i64 T, const i64 *targets, i64 m, double tol, i64 samples, u64 seed, u64 *out,
                             const SxwPlan &plan, void *ws, hipStream_t s) {
    using C = SxwCfg<D>;
    const i64 TT = T > 0 ? T : 1;
    const i64 pairs = plan.pairs, batch = plan.batch;               // batch >= 1: the caller asked
    char *w = (char *)align_up((size_t)ws, SxwPlan::ALIGN);
    int *cmem = (int *)(w + plan.cmem), *reci = (int *)(w + plan.reci);
    double *recd = (double *)(w + plan.recd), *m1g = (double *)(w + plan.m1g);
    SD_HIP(hipMemsetAsync(cmem, 0, (size_t)n * 4, s));
    hipLaunchKernelGGL(sxw_members_kernel, dim3((unsigned)((samples + 255) / 256)), dim3(256), 0, s, n, samples, seed, C::K, cmem);
    const i64 tiles = (m + 256 * C::TPT - 1) / (256 * C::TPT);
    for (i64 w0 = 0; w0 < pairs; w0 += batch) {
        const i64 cnt = pairs - w0 < batch ? pairs - w0 : batch;
        hipLaunchKernelGGL((sxw_factor_kernel<D>), dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, s, P, n, T, samples, seed, w0, cnt, recd, reci, m1g);
        i64 splits = (4096 + tiles - 1) / tiles;                        // about 4 096 workgroups in all
        if (splits > cnt) splits = cnt;
        if (splits > 65535) splits = 65535;
        hipLaunchKernelGGL((sxw_apply_kernel<D>), dim3((unsigned)tiles, (unsigned)splits), dim3(256), 0, s, P, n, T, targets, m, tol, samples,
                           seed, w0, cnt, (const double *)recd, (const int *)reci, out);
    }
    hipLaunchKernelGGL((sxw_spare_kernel<D>), dim3((unsigned)((m * TT + 255) / 256)), dim3(256), 0, s, P, n, T, targets, m, tol, samples, seed,
                       (const int *)cmem, out);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

static int launch_simplex_common(const double *P, i64 n, i64 T, int d, const PointSel &sel, i64 m, int relax,
                                 double tol, i64 samples, u64 seed, u64 *out, hipStream_t s, void *ws, size_t ws_bytes) {
    if (d < 1 || d > 8) return fail(SD_ERR_UNSUPPORTED, "simplex containment covers d in [1,8], got %d", d);
    SD_HIP(hipMemsetAsync(out, 0, sizeof(u64) * m, s));
    u64 total;
    if (samples >= 0) total = (u64)samples;                      // else the subsets of the most others a target has
    else if (!binom_u64_checked((u64)sel_others_max(sel, n), d + 1, &total)) return fail(SD_ERR_OVERFLOW, "subset count overflow");
    if (total == 0) return SD_OK;
    const bool generic = xswitch("SD_SIMPLEX_GENERIC") == 1;
    if (samples > 0 && !sel.members && !sel.Q && (T == 0 || relax) && n >= d + 3 && !generic && xswitch("SD_SIMPLEX_PERTARGET") != 1) {
        const SxwPlan plan = sxw_plan(n, T, d, samples, ws ? ws_bytes : 0);
        if (plan.batch > 0) {
            SD_DISPATCH_D(d, return launch_simplex_ws<D_>(P, n, T, sel.targets, m, tol, samples, seed, out, plan, ws, s))
        }
    }
    // aim for ~2^18 threads over all targets, at least 1 subset per thread
    u64 want_threads = ((u64)1 << 18) / (u64)(m > 0 ? m : 1);
    if (want_threads < SX_THREADS) want_threads = SX_THREADS;
    u64 per_thread = (total + want_threads - 1) / want_threads;
    if (per_thread < 1) per_thread = 1;
    u64 threads = (total + per_thread - 1) / per_thread;
    u64 blocks = (threads + SX_THREADS - 1) / SX_THREADS;
    if (blocks > 0x7fffffffull) return fail(SD_ERR_UNSUPPORTED, "too many subsets per target for one launch");
    for (i64 q0 = 0; q0 < m; q0 += 65535) {   // grid.y limit: fold large m into several launches
        i64 mm = m - q0 < 65535 ? m - q0 : 65535;
        dim3 grid((unsigned)blocks, (unsigned)mm);
        if (generic) {
            if (int rc = retired_simplex_generic(P, n, T, d, sel, relax, tol, total, per_thread, samples, seed, q0, out, grid, s)) return rc;
        } else {
            SD_DISPATCH_D(d, hipLaunchKernelGGL((simplex_kernel_fast<D_>), grid, dim3(SX_THREADS), 0, s, P, n, T, sel, relax,
                                                tol, total, per_thread, samples, seed, q0, out))
        }
    }
    SD_HIP(hipGetLastError());
    return SD_OK;
}

int launch_pointcloud_simplex(const double *P, i64 n, int d, const PointSel &sel, i64 m, double tol,
                              i64 samples, u64 seed, u64 *out, hipStream_t s, void *ws, size_t ws_bytes) {
    return launch_simplex_common(P, n, 0, d, sel, m, 1, tol, samples, seed, out, s, ws, ws_bytes);
}

int launch_multi_simplex(const double *P, i64 n, i64 T, int d, const i64 *targets, i64 m, int relax,
                         double tol, i64 samples, u64 seed, u64 *out, hipStream_t s, void *ws, size_t ws_bytes) {
    return launch_simplex_common(P, n, T, d, select_rows(targets), m, relax, tol, samples, seed, out, s, ws, ws_bytes);
}

}  // namespace sd
