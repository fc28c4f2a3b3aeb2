// halfspace_exact.hip -- K11: exact halfspace (Tukey) depth of a point cloud in the plane.
//
// Definition (include/statdepth_hip.h, K11).  Target q, sample points p_i, v_i = (fl(p_i0 - q0), fl(p_i1 - q1)), one
// rounded fp64 subtraction per component; c0 = #{v_i = (0, 0)} (q itself when it is a row; +1 for an external q).  With the
// EXACT signs of cross(a, b) = a0 b1 - a1 b0 and dot(a, b) = a0 b0 + a1 b1, for every nonzero v_j over the nonzero v_k:
//   L_j = #{cross(v_j, v_k) > 0}, R_j = #{cross < 0}, S_j = #{cross = 0, dot > 0} (j included), O_j = #{cross = 0, dot < 0},
//   out[q] = c0 + min_j min(L_j + O_j, R_j + S_j, L_j + S_j, R_j + O_j)        (c0 when no v is nonzero).
// The four candidates are the open sides of the line through q along v_j turned a hair to either side; the closed-halfplane
// count is upper semicontinuous in the direction, so its minimum over all closed halfplanes through q is reached there.
//
// Predicate.  sign(a b - c d): p1 = fl(a b), p2 = fl(c d); rounding is monotone, so p1 != p2 decides.  Otherwise the
// products' rounding errors e1 = fma(a, b, -p1), e2 = fma(c, d, -p2) are exact fp64 numbers and a b - c d = e1 - e2, so the
// comparison of e1 with e2 decides.  Exact while no product overflows or underflows: |coordinates| <= 2^500 (the host
// checks) and nonzero coordinate differences >= 2^-500 in magnitude (not checked: they are not known before they are formed).
//
// Two kernels over one selector (PointSel, point_select.h: a row of P against all rows; an external Q[q] against all rows
// with one added to c0; a block's last member against the block's members), the same integers from both:
//
// hx_sweep_kernel<CAP, NT>   one workgroup per target or block, samples of up to CAP = 64 / 512 / 2048 / 8192 points with
//   NT = 64 / 256 / 512 / 1024 threads.  The sample is streamed once: v formed, the nonzero vectors compacted into LDS (wave
//   ballot + one LDS atomic per wave) as they are, 16 bytes each in two fp64 arrays (consecutive lanes on consecutive
//   8-byte slots: no bank conflict in ds_read_b64 / ds_write_b64).  A vector is read through its image in the half-plane
//   y > 0 or (y = 0, x > 0): negated when the flag f(v) = (y < 0 or (y = 0 and x < 0)) is set -- negation is exact and f is
//   recomputed wherever it is needed, never stored.  The images are sorted by angle with a bitonic network whose comparator
//   is the exact cross sign (a total preorder on a half-plane; padding slots hold (0, 0), which no real element is, and sort
//   last).  rank_sort.h's network was not reused: its comparator is v_min_f64 / v_max_f64 on fp64 keys in registers, and
//   here the order has no fp64 key.  Cuts lie after the last element and wherever two neighbours have cross != 0; for a cut
//   after position s, A = #{i <= s, f = 0} + #{i > s, f = 1} and B = (number of nonzero vectors) - A.  The flags are prefix-
//   summed by ballot per run of 64 positions plus one wave scan over the runs; out = c0 + min over cuts of min(A, B).
//   LDS at CAP = 8192: 128 KiB of vectors + 528 bytes, one workgroup per CU.
//
// hx_pairwise_kernel   the definition taken literally: one workgroup of 256 threads per (target, 256 values of j), a thread
//   owns v_j in registers, every v_k passes through LDS in tiles of 256 (formed on load, read by every lane at the same
//   address: broadcast) -- O(n^2) predicate pairs per target.  Every workgroup counts c0 itself; the minimum over j goes
//   to out[q] with a 64-bit atomicMin (out is preset to all ones).  The independent cross-check of the sweep, and the route
//   for samples above 8192 points.
//
// Bounded launches: a sweep launch covers at most 2^34 comparator evaluations, a pairwise launch at most 2^36 predicate
// pairs or one workgroup (256 x n pairs; the 10^14 cap of the entry points keeps n below 10^7 on that route).
#include "sd_common.h"
#include "point_select.h"

namespace sd {

constexpr int HX_PT = 256;                                         // pairwise: threads, values of j per workgroup, tile
constexpr double HX_SWEEP_LAUNCH = 17179869184.0;                  // 2^34 comparator evaluations per sweep launch
constexpr double HX_PAIR_LAUNCH = 68719476736.0;                   // 2^36 predicate pairs per pairwise launch
constexpr int HX_NONE = 0x7fffffff;

// exact sign of a b - c d (see the header of this file)
__device__ __forceinline__ int hx_sign_diff(double a, double b, double c, double d) {
    const double p1 = __dmul_rn(a, b), p2 = __dmul_rn(c, d);
    if (p1 != p2) return p1 > p2 ? 1 : -1;
    const double e1 = __fma_rn(a, b, -p1), e2 = __fma_rn(c, d, -p2);
    return e1 > e2 ? 1 : (e1 < e2 ? -1 : 0);
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

__device__ __forceinline__ int hx_wave_min(int v) {
    for (int o = 32; o > 0; o >>= 1) {
        const int y = __shfl_down(v, o);
        v = y < v ? y : v;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------- sweep
template <int CAP, int NT>
__global__ __launch_bounds__(NT) void hx_sweep_kernel(const double *__restrict__ P, i64 n, PointSel sel, i64 q0,
                                                      i64 *__restrict__ out) {
    static_assert(CAP % 64 == 0 && NT % 64 == 0 && CAP / 64 <= 128, "one wave scans the runs of 64, two per lane at most");
    __shared__ double sx[CAP];
    __shared__ double sy[CAP];
    __shared__ int s_run[CAP / 64];                                 // flags set per run of 64 positions, then their prefix
    __shared__ int s_cnt, s_nz, s_min, s_t1;
    const int t = threadIdx.x, lane = t & 63;
    const i64 q = q0 + blockIdx.x;
    const PointView w = point_view_coop<NT>(sel, P, n, 2, q, &s_cnt);
    const double qx = w.x[0], qy = w.x[1];
    const int wcnt = (int)w.cnt;                                    // <= CAP: the launcher chose the tier
    if (t == 0) {
        s_nz = 0;
        s_min = HX_NONE;
    }
    __syncthreads();
    for (int i0 = 0; i0 < wcnt; i0 += NT) {                         // compaction of the nonzero vectors, in any order
        const int i = i0 + t;
        double vx = 0.0, vy = 0.0;
        if (i < wcnt) {
            const i64 src = w.mem ? (i64)w.mem[i] : (i64)i;
            vx = __dsub_rn(P[src * 2], qx);
            vy = __dsub_rn(P[src * 2 + 1], qy);
        }
        const bool nz = vx != 0.0 || vy != 0.0;
        const u64 mask = __ballot(nz);
        int base = 0;
        if (lane == 0 && mask) base = atomicAdd(&s_nz, __popcll(mask));
        base = __shfl(base, 0);
        if (nz) {
            const int pos = base + __popcll(mask & (((u64)1 << lane) - 1));
            sx[pos] = vx;
            sy[pos] = vy;
        }
    }
    __syncthreads();
    const int cnt = s_nz;
    const int c0 = wcnt - cnt + w.self();
    if (cnt == 0) {                                                 // (block-uniform) also the empty block: 0
        if (t == 0) out[q] = (i64)c0;
        return;
    }
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
    // F1(s) = #{i <= s : f}: per run of 64 positions by ballot, the runs by one wave
    for (int i0 = 0; i0 < cnt; i0 += NT) {
        const int i = i0 + t;
        const bool f = i < cnt && hx_flip(sx[i], sy[i]);
        const u64 mask = __ballot(f);
        if (lane == 0 && i < cnt) s_run[i >> 6] = __popcll(mask);
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
        if (t == 63) s_t1 = inc;
    }
    __syncthreads();
    const int T1 = s_t1;
    int best = HX_NONE;
    for (int i0 = 0; i0 < cnt; i0 += NT) {
        const int i = i0 + t;
        double ax = 0.0, ay = 0.0;
        if (i < cnt) {
            ax = sx[i];
            ay = sy[i];
        }
        const bool f = i < cnt && hx_flip(ax, ay);
        const u64 mask = __ballot(f);
        if (i < cnt && (i == cnt - 1 || hx_cross(ax, ay, sx[i + 1], sy[i + 1]) != 0)) {
            const int F1 = s_run[i >> 6] + __popcll(mask & (((u64)2 << lane) - 1));
            const int A = (i + 1 - F1) + (T1 - F1);
            const int B = cnt - A;
            const int c = A < B ? A : B;
            best = c < best ? c : best;
        }
    }
    best = hx_wave_min(best);
    if (lane == 0 && best != HX_NONE) atomicMin(&s_min, best);
    __syncthreads();
    if (t == 0) out[q] = (i64)c0 + (i64)s_min;
}

static inline double hx_sweep_wg_work(int cap) {                    // comparator evaluations of one workgroup at a tier
    int L = 0;
    while ((1 << L) < cap) ++L;
    return (double)(cap / 2) * (double)(L * (L + 1) / 2);
}

static inline int hx_tier(i64 cnt_max) { return cnt_max <= 64 ? 64 : cnt_max <= 512 ? 512 : cnt_max <= 2048 ? 2048 : 8192; }

template <int CAP, int NT>
static int hx_launch_sweep(const double *P, i64 n, const PointSel &sel, i64 m, i64 *out, hipStream_t s) {
    double per = HX_SWEEP_LAUNCH / hx_sweep_wg_work(CAP);
    per = per > 1048576.0 ? 1048576.0 : per;
    const i64 g = (i64)per;
    for (i64 q0 = 0; q0 < m; q0 += g) {
        const i64 mb = m - q0 < g ? m - q0 : g;
        hipLaunchKernelGGL((hx_sweep_kernel<CAP, NT>), dim3((unsigned)mb), dim3(NT), 0, s, P, n, sel, q0, out);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------- pairwise
// unit = u0 + blockIdx.x = (target q) * C + (chunk c of 256 values of j)
__global__ __launch_bounds__(HX_PT) void hx_pairwise_kernel(const double *__restrict__ P, i64 n, PointSel sel, u64 u0, u64 C,
                                                            unsigned long long *__restrict__ out) {
    __shared__ double tx[HX_PT];
    __shared__ double ty[HX_PT];
    __shared__ int s_cnt, s_zero, s_min;
    const int t = threadIdx.x;
    const u64 u = u0 + blockIdx.x;
    const i64 q = (i64)(u / C);
    const i64 c = (i64)(u % C);
    const PointView w = point_view_coop<HX_PT>(sel, P, n, 2, q, &s_cnt);
    const double qx = w.x[0], qy = w.x[1];
    const int wcnt = (int)w.cnt;
    if (c > 0 && c * HX_PT >= wcnt) return;                         // (block-uniform) a shorter block of the members form
    if (t == 0) {
        s_zero = 0;
        s_min = HX_NONE;
    }
    const i64 j = c * HX_PT + t;
    double jx = 0.0, jy = 0.0;
    if (j < wcnt) {
        const i64 src = w.mem ? (i64)w.mem[j] : j;
        jx = __dsub_rn(P[src * 2], qx);
        jy = __dsub_rn(P[src * 2 + 1], qy);
    }
    const bool active = jx != 0.0 || jy != 0.0;
    u32 L = 0, R = 0, S = 0, O = 0;
    int zeros = 0;
    for (i64 k0 = 0; k0 < wcnt; k0 += HX_PT) {
        const int tc = (int)(wcnt - k0 < HX_PT ? wcnt - k0 : HX_PT);
        __syncthreads();
        if (t < tc) {
            const i64 src = w.mem ? (i64)w.mem[k0 + t] : k0 + t;
            const double vx = __dsub_rn(P[src * 2], qx);
            const double vy = __dsub_rn(P[src * 2 + 1], qy);
            tx[t] = vx;
            ty[t] = vy;
            zeros += vx == 0.0 && vy == 0.0 ? 1 : 0;
        }
        __syncthreads();
        if (active) {
            for (int k = 0; k < tc; ++k) {
                const double bx = tx[k], by = ty[k];                // every lane the same address: broadcast
                const int sc = hx_cross(jx, jy, bx, by);
                if (sc > 0) ++L;
                else if (sc < 0) ++R;
                else {                                              // a zero v_k lands here and counts nowhere
                    const int sd = hx_dot(jx, jy, bx, by);
                    S += sd > 0 ? 1u : 0u;
                    O += sd < 0 ? 1u : 0u;
                }
            }
        }
    }
    if (zeros) atomicAdd(&s_zero, zeros);
    int best = HX_NONE;
    if (active) {
        const u32 a = L + O < R + S ? L + O : R + S;
        const u32 b = L + S < R + O ? L + S : R + O;
        best = (int)(a < b ? a : b);
    }
    best = hx_wave_min(best);
    if ((t & 63) == 0 && best != HX_NONE) atomicMin(&s_min, best);
    __syncthreads();
    if (t == 0) {
        const int c0 = s_zero + w.self();
        if (s_zero == wcnt) {                                       // no nonzero vector (also the empty block: 0)
            if (c == 0) atomicMin(&out[q], (unsigned long long)c0);
        } else if (s_min != HX_NONE) {
            atomicMin(&out[q], (unsigned long long)c0 + (unsigned long long)s_min);
        }
    }
}

static int hx_launch_pairwise(const double *P, i64 n, const PointSel &sel, i64 m, i64 *out, hipStream_t s) {
    const i64 cnt_max = sel_cnt_max(sel, n);
    const u64 C = (u64)((cnt_max + HX_PT - 1) / HX_PT);
    SD_HIP(hipMemsetAsync(out, 0xff, (size_t)m * 8, s));
    double per = HX_PAIR_LAUNCH / ((double)HX_PT * (double)cnt_max);
    per = per < 1.0 ? 1.0 : per > 1048576.0 ? 1048576.0 : per;
    const u64 g = (u64)per;
    const u64 units = (u64)m * C;
    for (u64 u0 = 0; u0 < units; u0 += g) {
        const u64 ub = units - u0 < g ? units - u0 : g;
        hipLaunchKernelGGL(hx_pairwise_kernel, dim3((unsigned)ub), dim3(HX_PT), 0, s, P, n, sel, u0, C,
                           (unsigned long long *)out);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------- routes
// The route of a call (1 = sweep, 2 = pairwise) whose largest sample has cnt_max points; 0: algo = 1 above the capacity.
// Auto: the sweep wherever it fits -- profiles/halfspace_exact_times.txt has it ahead of the pairwise kernel at every size
// measured.
int halfspace2_route(int algo, i64 cnt_max) {
    if (algo == 2) return 2;
    if (cnt_max <= HX_SWEEP_CAPACITY) return 1;
    return algo == 1 ? 0 : 2;
}

// predicate evaluations of the call on that route
double halfspace2_work(int route, i64 m, i64 cnt_max) {
    if (route == 2) return (double)m * (double)cnt_max * (double)cnt_max;
    return (double)m * hx_sweep_wg_work(hx_tier(cnt_max));
}

int launch_halfspace2(const double *P, i64 n, const PointSel &sel, i64 m, int route, i64 *out, hipStream_t s) {
    if (route == 2) return hx_launch_pairwise(P, n, sel, m, out, s);
    switch (hx_tier(sel_cnt_max(sel, n))) {
        case 64: return hx_launch_sweep<64, 64>(P, n, sel, m, out, s);
        case 512: return hx_launch_sweep<512, 256>(P, n, sel, m, out, s);
        case 2048: return hx_launch_sweep<2048, 512>(P, n, sel, m, out, s);
    }
    return hx_launch_sweep<8192, 1024>(P, n, sel, m, out, s);
}

}  // namespace sd
