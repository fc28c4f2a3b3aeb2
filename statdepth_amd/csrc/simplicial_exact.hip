// simplicial_exact.hip -- K13: exact simplicial depth of a point cloud in the plane by angular sweep.
//
// Definition (include/statdepth_hip.h, K13).  Target x, its others p_i (the sample without the target's own row, m of
// them), v_i = (fl(p_i0 - x0), fl(p_i1 - x1)), one rounded fp64 subtraction per component.  With the EXACT signs of
// cross(a, b) = a0 b1 - a1 b0 and dot(a, b) = a0 b0 + a1 b1 (plane_sweep.h), for every nonzero v_j over the nonzero v_k:
//   e_j = #{k : cross(v_j, v_k) > 0} + #{k later than j among the others : cross(v_j, v_k) = 0 and dot(v_j, v_k) > 0},
//   out[x] = C(m, 3) - sum_j C(e_j, 2).
// A triple of others misses x exactly when its three vectors are nonzero and fit in an open half-plane; such a triple has
// one clockwise-most member j (members of one direction ordered by position), the other two are among j's e_j, and every
// pair of those e_j forms such a triple with j: sum_j C(e_j, 2) counts the missing triples once each.  The sum does not
// depend on the order inside a direction class: over a class of size s with common L = #{cross > 0} it is
// sum_{r < s} C(L + r, 2).
//
// Two kernels over one selector (PointSel, point_select.h; the target's OTHERS are the vectors), the same integers from both:
//
// sx2_sweep_kernel<CAP, NT>   one workgroup per target or block, up to CAP = 64 / 512 / 2048 / 8192 others with NT = 64 /
//   256 / 512 / 1024 threads.  Compaction, sort and flag prefix are K11's (plane_sweep.h).  Groups are runs of sorted
//   neighbours with cross = 0: one direction and its opposite, told apart by the flip flag.  The element at position i of
//   group [g0, g1] with flag f has L = #{positions > g1 with flag f} + #{positions < g0 with flag != f} and rank r = its
//   index among the same-flag elements of its group, all three from the flag prefix F: with Fx(p) = #{flags below p},
//     f = 1: L = (T1 - Fx(g1 + 1)) + (g0 - Fx(g0)),                  r = Fx(i) - Fx(g0)
//     f = 0: L = ((cnt - 1 - g1) - (T1 - Fx(g1 + 1))) + Fx(g0),      r = (i - g0) - (Fx(i) - Fx(g0)).
//   Group starts are one 64-bit mask per run of 64 positions; g0 and g1 are bit scans inside the run, and where the run has
//   no start at or below (above) the position, the last start before the run (the first after it), which one wave finds
//   for every run by a max (min) scan.  No loop runs over a group.  C(L + r, 2) accumulates in 64 bits (one term is at
//   most C(8191, 2), the sum at most C(8192, 3)), is reduced over the workgroup, and thread 0 writes C(m, 3) - sum.
//   LDS at CAP = 8192: 128 KiB of vectors + 3.7 KiB (flag and start masks, flag prefix, the two carries), one workgroup per CU.
//
// sx2_pairwise_kernel   the definition taken literally: one workgroup of 256 threads per (target, 256 values of j), a thread
//   owns v_j in registers, every v_k passes through LDS in tiles of 256 (formed on load, read by every lane at the same
//   address: broadcast) -- O(m^2) predicate pairs per target.  The workgroup's sum of C(e_j, 2) is added to out[x] (preset
//   to 0) with one 64-bit atomicAdd; sx2_finalize_kernel then turns the sum into C(m, 3) - sum.  The independent
//   cross-check of the sweep, and the route above 8192 others.
//
// Bounded launches, as K11's: a sweep launch covers at most 2^34 comparator evaluations, a pairwise launch at most 2^36
// predicate pairs or one workgroup (256 x m pairs).
#include "sd_common.h"
#include "point_select.h"
#include "plane_sweep.h"

namespace sd {

constexpr int SX_PT = 256;                                         // pairwise: threads, values of j per workgroup, tile
constexpr double SX_SWEEP_LAUNCH = 17179869184.0;                  // 2^34 comparator evaluations per sweep launch
constexpr double SX_PAIR_LAUNCH = 68719476736.0;                   // 2^36 predicate pairs per pairwise launch
constexpr int SX_NONE = 0x7fffffff;

// C(a, 3) without an intermediate above the result: one of a, a - 1, a - 2 is a multiple of 3
__device__ __forceinline__ u64 sx2_choose3(u64 a) {
    if (a < 3) return 0;
    const u64 c2 = a * (a - 1) / 2;
    return (a - 2) % 3 == 0 ? c2 * ((a - 2) / 3) : c2 / 3 * (a - 2);
}

__device__ __forceinline__ u64 sx2_wave_sum(u64 v) {
    for (int o = 32; o > 0; o >>= 1) v += (u64)__shfl_down((unsigned long long)v, o);
    return v;
}

// ---------------------------------------------------------------------------------------------- sweep
template <int CAP, int NT>
__global__ __launch_bounds__(NT) void sx2_sweep_kernel(const double *__restrict__ P, i64 n, PointSel sel, i64 q0,
                                                       i64 *__restrict__ out) {
    constexpr int RUNS = CAP / 64;
    __shared__ double sx[CAP];
    __shared__ double sy[CAP];
    __shared__ u64 s_flags[RUNS];                                   // flip flags per run of 64 positions
    __shared__ u64 s_start[RUNS];                                   // group starts per run
    __shared__ int s_run[RUNS];                                     // flags set before the run
    __shared__ int s_prev[RUNS];                                    // the last group start before the run
    __shared__ int s_next[RUNS];                                    // the first group start after the run, cnt if none
    __shared__ u64 s_part[NT / 64];
    __shared__ int s_cnt, s_nz, s_t1;
    const int t = threadIdx.x, lane = t & 63;
    const i64 q = q0 + blockIdx.x;
    const PointView w = point_view_coop<NT>(sel, P, n, 2, q, &s_cnt);
    const u64 total = sx2_choose3((u64)w.others());                 // others() <= CAP: the launcher chose the tier
    const int cnt = hx_compact<NT, true>(P, w, sx, sy, &s_nz);
    if (cnt == 0) {                                                 // (block-uniform) every triple holds a duplicate of x
        if (t == 0) out[q] = (i64)total;
        return;
    }
    hx_sort<NT>(sx, sy, cnt);
    const int T1 = hx_flag_prefix<CAP, NT>(sx, sy, cnt, s_run, &s_t1, s_flags);
    const int nrun = (cnt + 63) >> 6;
    for (int i0 = 0; i0 < cnt; i0 += NT) {                          // group starts: position 0 and wherever cross != 0
        const int i = i0 + t;
        const bool st = i < cnt && (i == 0 || hx_cross(sx[i - 1], sy[i - 1], sx[i], sy[i]) != 0);
        const u64 mask = __ballot(st);
        if (lane == 0 && i < cnt) s_start[i >> 6] = mask;
    }
    __syncthreads();
    if (t < 64) {                                                   // the carries across runs: a max and a min scan
        constexpr int EPL = (RUNS + 63) / 64;                       // runs per lane
        int hi[EPL], lo[EPL], lmax = -1, lmin = SX_NONE;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int r = t * EPL + e;
            const u64 b = r < nrun ? s_start[r] : 0;
            hi[e] = b ? r * 64 + 63 - __clzll((long long)b) : -1;
            lo[e] = b ? r * 64 + __ffsll((unsigned long long)b) - 1 : SX_NONE;
            lmax = hi[e] > lmax ? hi[e] : lmax;
            lmin = lo[e] < lmin ? lo[e] : lmin;
        }
        int pmax = lmax, smin = lmin;
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(pmax, o), z = __shfl_down(smin, o);
            if (t >= o) pmax = y > pmax ? y : pmax;
            if (t + o < 64) smin = z < smin ? z : smin;
        }
        int before = __shfl_up(pmax, 1), after = __shfl_down(smin, 1);
        if (t == 0) before = -1;
        if (t == 63) after = SX_NONE;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const int r = t * EPL + e;
            if (r < nrun) s_prev[r] = before;
            before = hi[e] > before ? hi[e] : before;
        }
#pragma unroll
        for (int e = EPL - 1; e >= 0; --e) {
            const int r = t * EPL + e;
            if (r < nrun) s_next[r] = after < cnt ? after : cnt;
            after = lo[e] < after ? lo[e] : after;
        }
    }
    __syncthreads();
    u64 sum = 0;
    for (int i0 = 0; i0 < cnt; i0 += NT) {
        const int i = i0 + t;
        if (i < cnt) {
            const int r = i >> 6;
            const u64 b = s_start[r], fl = s_flags[r];
            const u64 upto = ((u64)2 << lane) - 1;                  // bits 0 .. lane (lane 63: all)
            const u64 below = b & upto, above = b & ~upto;
            const int g0 = below ? r * 64 + 63 - __clzll((long long)below) : s_prev[r];   // run 0 has bit 0 set
            const int g1 = (above ? r * 64 + __ffsll((unsigned long long)above) - 1 : s_next[r]) - 1;
            const bool f = (fl >> lane) & 1;
            const int Fi = s_run[r] + __popcll(fl & (((u64)1 << lane) - 1));
            const int Fg0 = s_run[g0 >> 6] + __popcll(s_flags[g0 >> 6] & (((u64)1 << (g0 & 63)) - 1));
            const int Fg1 = s_run[g1 >> 6] + __popcll(s_flags[g1 >> 6] & (((u64)2 << (g1 & 63)) - 1));   // through g1
            const int L = f ? (T1 - Fg1) + (g0 - Fg0) : ((cnt - 1 - g1) - (T1 - Fg1)) + Fg0;
            const int rk = f ? Fi - Fg0 : (i - g0) - (Fi - Fg0);
            const u64 e = (u64)(L + rk);
            sum += e * (e - 1) / 2;                                 // e = 0: 0 * (2^64 - 1) / 2 = 0
        }
    }
    sum = sx2_wave_sum(sum);
    if (lane == 0) s_part[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
        u64 all = 0;
        for (int v = 0; v < NT / 64; ++v) all += s_part[v];
        out[q] = (i64)(total - all);
    }
}

template <int CAP, int NT>
static int sx2_launch_sweep(const double *P, i64 n, const PointSel &sel, i64 m, i64 *out, hipStream_t s) {
    double per = SX_SWEEP_LAUNCH / hx_sweep_wg_work(CAP);
    per = per > 1048576.0 ? 1048576.0 : per;
    const i64 g = (i64)per;
    for (i64 q0 = 0; q0 < m; q0 += g) {
        const i64 mb = m - q0 < g ? m - q0 : g;
        hipLaunchKernelGGL((sx2_sweep_kernel<CAP, NT>), dim3((unsigned)mb), dim3(NT), 0, s, P, n, sel, q0, out);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------- pairwise
// unit = u0 + blockIdx.x = (target q) * C + (chunk c of 256 values of j)
__global__ __launch_bounds__(SX_PT) void sx2_pairwise_kernel(const double *__restrict__ P, i64 n, PointSel sel, u64 u0, u64 C,
                                                             unsigned long long *__restrict__ out) {
    __shared__ double tx[SX_PT];
    __shared__ double ty[SX_PT];
    __shared__ u64 s_part[SX_PT / 64];
    __shared__ int s_cnt;
    const int t = threadIdx.x;
    const u64 u = u0 + blockIdx.x;
    const i64 q = (i64)(u / C);
    const i64 c = (i64)(u % C);
    const PointView w = point_view_coop<SX_PT>(sel, P, n, 2, q, &s_cnt);
    const double qx = w.x[0], qy = w.x[1];
    const i64 m = w.others();
    if (c * SX_PT >= m) return;                                     // (block-uniform) fewer others than the call's most
    const i64 j = c * SX_PT + t;
    double jx = 0.0, jy = 0.0;
    if (j < m) {
        const i64 src = w.other(j);
        jx = __dsub_rn(P[src * 2], qx);
        jy = __dsub_rn(P[src * 2 + 1], qy);
    }
    const bool active = jx != 0.0 || jy != 0.0;
    u64 e = 0;
    for (i64 k0 = 0; k0 < m; k0 += SX_PT) {
        const int tc = (int)(m - k0 < SX_PT ? m - k0 : SX_PT);
        __syncthreads();
        if (t < tc) {
            const i64 src = w.other(k0 + t);
            tx[t] = __dsub_rn(P[src * 2], qx);
            ty[t] = __dsub_rn(P[src * 2 + 1], qy);
        }
        __syncthreads();
        if (active) {
            for (int k = 0; k < tc; ++k) {
                const double bx = tx[k], by = ty[k];                // every lane the same address: broadcast
                const int sc = hx_cross(jx, jy, bx, by);
                if (sc > 0) ++e;
                else if (sc == 0 && k0 + k > j && hx_dot(jx, jy, bx, by) > 0) ++e;   // a zero v_k has dot = 0
            }
        }
    }
    u64 sum = sx2_wave_sum(e * (e - 1) / 2);                        // e = 0 (also an inactive thread): 0
    if ((t & 63) == 0) s_part[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
        sum = 0;
        for (int v = 0; v < SX_PT / 64; ++v) sum += s_part[v];
        if (sum) atomicAdd(&out[q], (unsigned long long)sum);
    }
}

// out[q] holds sum_j C(e_j, 2): C(m, 3) - that
__global__ __launch_bounds__(256) void sx2_finalize_kernel(const double *__restrict__ P, i64 n, PointSel sel, i64 q0, i64 m,
                                                           i64 *out) {
    const i64 q = q0 + (i64)blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    const PointView w = point_view(sel, P, n, 2, q);
    out[q] = (i64)(sx2_choose3((u64)w.others()) - (u64)out[q]);
}

static int sx2_launch_pairwise(const double *P, i64 n, const PointSel &sel, i64 m, i64 *out, hipStream_t s) {
    const i64 others_max = sel_others_max(sel, n);
    SD_HIP(hipMemsetAsync(out, 0, (size_t)m * 8, s));
    if (others_max >= 3) {                                          // fewer: no triple, the sums stay 0
        const u64 C = (u64)((others_max + SX_PT - 1) / SX_PT);
        double per = SX_PAIR_LAUNCH / ((double)SX_PT * (double)others_max);
        per = per < 1.0 ? 1.0 : per > 1048576.0 ? 1048576.0 : per;
        const u64 g = (u64)per;
        const u64 units = (u64)m * C;
        for (u64 u0 = 0; u0 < units; u0 += g) {
            const u64 ub = units - u0 < g ? units - u0 : g;
            hipLaunchKernelGGL(sx2_pairwise_kernel, dim3((unsigned)ub), dim3(SX_PT), 0, s, P, n, sel, u0, C,
                               (unsigned long long *)out);
            SD_HIP(hipGetLastError());
        }
    }
    const i64 g = (i64)1 << 28;                                     // 2^20 workgroups of 256 targets per launch
    for (i64 q0 = 0; q0 < m; q0 += g) {
        const i64 mb = m - q0 < g ? m - q0 : g;
        hipLaunchKernelGGL(sx2_finalize_kernel, dim3((unsigned)((mb + 255) / 256)), dim3(256), 0, s, P, n, sel, q0, m, out);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------- routes
// The route of a call (1 = sweep, 2 = pairwise) whose targets have at most others_max others; 0: algo = 1 above the
// capacity.  Auto: the sweep wherever it fits.
int simplicial2_route(int algo, i64 others_max) {
    if (algo == 2) return 2;
    if (others_max <= SX_SWEEP_CAPACITY) return 1;
    return algo == 1 ? 0 : 2;
}

// predicate evaluations of the call on that route (K11's formulas over the others)
double simplicial2_work(int route, i64 m, i64 others_max) {
    if (route == 2) return (double)m * (double)others_max * (double)others_max;
    return (double)m * hx_sweep_wg_work(hx_tier(others_max));
}

// the most others whose C(others, 3) fits int64
i64 simplicial2_max_others() {
    i64 lo = 3, hi = (i64)1 << 31;                                  // C(lo, 3) fits, C(hi, 3) does not
    while (hi - lo > 1) {
        const i64 mid = lo + (hi - lo) / 2;
        u64 v = 0;
        if (binom_u64_checked((u64)mid, 3, &v) && v <= (u64)INT64_MAX) lo = mid;
        else hi = mid;
    }
    return lo;
}

int launch_simplicial2(const double *P, i64 n, const PointSel &sel, i64 m, int route, i64 *out, hipStream_t s) {
    if (route == 2) return sx2_launch_pairwise(P, n, sel, m, out, s);
    switch (hx_tier(sel_others_max(sel, n))) {
        case 64: return sx2_launch_sweep<64, 64>(P, n, sel, m, out, s);
        case 512: return sx2_launch_sweep<512, 256>(P, n, sel, m, out, s);
        case 2048: return sx2_launch_sweep<2048, 512>(P, n, sel, m, out, s);
    }
    return sx2_launch_sweep<8192, 1024>(P, n, sel, m, out, s);
}

}  // namespace sd
