// plane_sweep.h -- the angular sweep around one point of a planar cloud, shared by K11 (halfspace_exact.hip) and K13
// (simplicial_exact.hip) (internal, device code).
//
// Predicate.  sign(a b - c d): p1 = fl(a b), p2 = fl(c d); rounding is monotone, also where it is subnormal or flushes to
// zero, so p1 != p2 decides.  Otherwise a b - c d = e1 - e2 with the products' rounding errors e1 = a b - p1, e2 = c d - p2,
// and e = fma(a, b, -p) is that error whenever it is an fp64 number.  It is a multiple of ulp(a) ulp(b) > |a b| 2^-106 (the
// ulp of a subnormal is 2^-1074) of magnitude at most ulp(p) / 2, so it is one while |p| >= 2^-900: ulp(a) ulp(b) is then
// above 2^-1007.  Below that (the products of tiny differences; also p1 = p2 = 0, where the errors ARE the products, and
// e1 = u^2 2^-972 was lost from the witness of tests/test_planar_scale_host.py) nothing is left to the fma: a zero operand
// is settled by the signs of the other product; otherwise frexp takes the four operands to mantissas in [1/2, 1) (exact,
// subnormals included), differing signs of the products decide, exponent sums two or more apart decide (a product of two
// mantissas lies in [1/4, 1)), and the remaining case is the same two-branch comparison on the mantissas, one of them times
// 2^-1, 2^0 or 2^1, where every product is in [1/8, 2) and no error can be lost.  So the sign is exact for every finite
// a, b, c, d whose products do not overflow: |coordinates| <= 2^500 (the host checks; differences are then at most 2^501
// and products at most 2^1002), with no lower limit on the differences.
//
// Sweep.  The vectors v_i = (fl(p_i0 - q0), fl(p_i1 - q1)) from the target q to its sample are streamed once, the nonzero
// ones compacted into LDS (wave ballot + one LDS atomic per wave) as they are, 16 bytes each in two fp64 arrays (consecutive
// lanes on consecutive 8-byte slots: no bank conflict in ds_read_b64 / ds_write_b64).  A vector is read through its image in
// the half-plane y > 0 or (y = 0, x > 0): negated when the flag f(v) = (y < 0 or (y = 0 and x < 0)) is set -- negation is
// exact and f is recomputed wherever it is needed, never stored.  The images are sorted by angle with a bitonic network
// whose comparator is the exact cross sign (a total preorder on a half-plane; padding slots hold (0, 0), which no real
// element is, and sort last).  rank_sort.h's network was not reused: its comparator is v_min_f64 / v_max_f64 on fp64 keys in
// registers, and here the order has no fp64 key.  The flags are prefix-summed by ballot per run of 64 positions plus one
// wave scan over the runs.
#pragma once
#include "sd_common.h"
#include "point_select.h"

namespace sd {

// comparator evaluations of one sweep workgroup at a capacity tier: (cap / 2) log2 cap (log2 cap + 1) / 2
static inline double hx_sweep_wg_work(int cap) {
    int L = 0;
    while ((1 << L) < cap) ++L;
    return (double)(cap / 2) * (double)(L * (L + 1) / 2);
}

// the capacity tier (vectors one sweep workgroup holds) of a call whose largest sample has cnt_max vectors
static inline int hx_tier(i64 cnt_max) { return cnt_max <= 64 ? 64 : cnt_max <= 512 ? 512 : cnt_max <= 2048 ? 2048 : 8192; }

#ifdef __HIPCC__
// sign(a b - c d) where fl(a b) = fl(c d) is below 2^-900 in magnitude and no operand is zero: by exponents and mantissas
static __device__ __noinline__ int hx_sign_diff_tiny(double a, double b, double c, double d) {
    int ea, eb, ec, ed;
    double ma = frexp(a, &ea);
    const double mb = frexp(b, &eb), mc = frexp(c, &ec), md = frexp(d, &ed);
    const int s1 = (ma < 0.0) != (mb < 0.0) ? -1 : 1, s2 = (mc < 0.0) != (md < 0.0) ? -1 : 1;
    if (s1 != s2) return s1;                                        // a b and c d on either side of zero
    const int de = (ea + eb) - (ec + ed);                           // |a b| in [2^(ea+eb-2), 2^(ea+eb)), c d likewise
    if (de >= 2) return s1;
    if (de <= -2) return -s1;
    ma = ldexp(ma, de);
    const double p1 = __dmul_rn(ma, mb), p2 = __dmul_rn(mc, md);
    if (p1 != p2) return p1 > p2 ? 1 : -1;
    const double e1 = __fma_rn(ma, mb, -p1), e2 = __fma_rn(mc, md, -p2);
    return e1 > e2 ? 1 : (e1 < e2 ? -1 : 0);
}

// exact sign of a b - c d (see the header of this file)
__device__ __forceinline__ int hx_sign_diff(double a, double b, double c, double d) {
    const double p1 = __dmul_rn(a, b), p2 = __dmul_rn(c, d);
    if (p1 != p2) return p1 > p2 ? 1 : -1;
    if (fabs(p1) >= 0x1p-900) {                                     // the errors are fp64 numbers
        const double e1 = __fma_rn(a, b, -p1), e2 = __fma_rn(c, d, -p2);
        return e1 > e2 ? 1 : (e1 < e2 ? -1 : 0);
    }
    const bool z1 = a == 0.0 || b == 0.0, z2 = c == 0.0 || d == 0.0;
    if (z1 || z2) {                                                 // a b - c d = - c d, a b or 0, by the signs alone
        if (z1 && z2) return 0;
        return z1 ? ((c < 0.0) != (d < 0.0) ? 1 : -1) : ((a < 0.0) != (b < 0.0) ? -1 : 1);
    }
    return hx_sign_diff_tiny(a, b, c, d);
}
__device__ __forceinline__ int hx_cross(double ax, double ay, double bx, double by) { return hx_sign_diff(ax, by, ay, bx); }
__device__ __forceinline__ int hx_dot(double ax, double ay, double bx, double by) { return hx_sign_diff(ax, bx, -ay, by); }

// the vector lies outside the half-plane y > 0 or (y = 0, x > 0): its image there is -v
__device__ __forceinline__ bool hx_flip(double x, double y) { return y < 0.0 || (y == 0.0 && x < 0.0); }

// a's image sorts strictly behind b's: by angle in [0, pi), padding (0, 0) behind every real element
__device__ __forceinline__ bool hx_after(double ax, double ay, double bx, double by) {
    const bool apad = ax == 0.0 && ay == 0.0, bpad = bx == 0.0 && by == 0.0;
    if (apad || bpad) return apad && !bpad;
    const int s = hx_cross(ax, ay, bx, by);
    return hx_flip(ax, ay) != hx_flip(bx, by) ? s > 0 : s < 0;
}

// Compaction: the nonzero vectors from w's target to its sample (OTHERS: to its others, the target's own row skipped) go
// to sx / sy[0 .. return value), in any order.  The caller chose the arrays to hold the whole sample.  Barriers inside:
// every thread of the workgroup calls it, and what thread 0 wrote to LDS before the call is visible after it.
template <int NT, bool OTHERS>
__device__ __forceinline__ int hx_compact(const double *__restrict__ P, const PointView &w, double *sx, double *sy, int *s_nz) {
    const int t = threadIdx.x, lane = t & 63;
    const double qx = w.x[0], qy = w.x[1];
    const int wcnt = (int)(OTHERS ? w.others() : w.cnt);
    if (t == 0) *s_nz = 0;
    __syncthreads();
    for (int i0 = 0; i0 < wcnt; i0 += NT) {
        const int i = i0 + t;
        double vx = 0.0, vy = 0.0;
        if (i < wcnt) {
            const i64 src = OTHERS ? w.other(i) : (w.mem ? (i64)w.mem[i] : (i64)i);
            vx = __dsub_rn(P[src * 2], qx);
            vy = __dsub_rn(P[src * 2 + 1], qy);
        }
        const bool nz = vx != 0.0 || vy != 0.0;
        const u64 mask = __ballot(nz);
        int base = 0;
        if (lane == 0 && mask) base = atomicAdd(s_nz, __popcll(mask));
        base = __shfl(base, 0);
        if (nz) {
            const int pos = base + __popcll(mask & (((u64)1 << lane) - 1));
            sx[pos] = vx;
            sy[pos] = vy;
        }
    }
    __syncthreads();
    return *s_nz;
}

// Bitonic sort of the images of sx / sy[0 .. cnt), cnt >= 1, by angle; the slots up to the next power of two are padded
// with (0, 0).  Ends with a barrier.
template <int NT>
__device__ __forceinline__ void hx_sort(double *sx, double *sy, int cnt) {
    const int t = threadIdx.x;
    int N2 = 2;
    while (N2 < cnt) N2 <<= 1;
    for (int p = cnt + t; p < N2; p += NT) {
        sx[p] = 0.0;
        sy[p] = 0.0;
    }
    __syncthreads();
    for (int k = 2; k <= N2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = t; x < (N2 >> 1); x += NT) {
                const int i = ((x & ~(j - 1)) << 1) | (x & (j - 1));
                const int l = i | j;
                const bool up = (i & k) == 0;
                const double ax = sx[i], ay = sy[i], bx = sx[l], by = sy[l];
                const bool sw = up ? hx_after(ax, ay, bx, by) : hx_after(bx, by, ax, ay);
                if (sw) {
                    sx[i] = bx; sy[i] = by;
                    sx[l] = ax; sy[l] = ay;
                }
            }
            __syncthreads();
        }
    }
}

// Flag prefix: s_run[r] = #{i < 64 r : f(i)} for the runs r of 64 positions below cnt, the total returned (through
// *s_t1); s_flags, where given, gets the flags of run r as a mask (bit b: position 64 r + b).  Ends with a barrier.
template <int CAP, int NT>
__device__ __forceinline__ int hx_flag_prefix(const double *sx, const double *sy, int cnt, int *s_run, int *s_t1,
                                              u64 *s_flags) {
    static_assert(CAP % 64 == 0 && NT % 64 == 0 && CAP / 64 <= 128, "one wave scans the runs of 64, two per lane at most");
    const int t = threadIdx.x, lane = t & 63;
    for (int i0 = 0; i0 < cnt; i0 += NT) {
        const int i = i0 + t;
        const bool f = i < cnt && hx_flip(sx[i], sy[i]);
        const u64 mask = __ballot(f);
        if (lane == 0 && i < cnt) {
            s_run[i >> 6] = __popcll(mask);
            if (s_flags) s_flags[i >> 6] = mask;
        }
    }
    __syncthreads();
    if (t < 64) {
        constexpr int EPL = (CAP / 64 + 63) / 64;                   // runs per lane
        const int nrun = (cnt + 63) >> 6;
        int v[EPL], sum = 0;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int r = t * EPL + e;
            v[e] = r < nrun ? s_run[r] : 0;
            sum += v[e];
        }
        int inc = sum;
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(inc, o);
            if (t >= o) inc += y;
        }
        int exc = inc - sum;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int r = t * EPL + e;
            if (r < nrun) s_run[r] = exc;
            exc += v[e];
        }
        if (t == 63) *s_t1 = inc;
    }
    __syncthreads();
    return *s_t1;
}
#endif

}  // namespace sd
