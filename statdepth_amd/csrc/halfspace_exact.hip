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
// The exact predicate, the compaction of the vectors into LDS, the angular sort of their half-plane images and the flag
// prefix are plane_sweep.h, shared with K13 (simplicial_exact.hip).
//
// Two kernels over one selector (PointSel, point_select.h: a row of P against all rows; an external Q[q] against all rows
// with one added to c0; a block's last member against the block's members), the same integers from both:
//
// hx_sweep_kernel<CAP, NT>   one workgroup per target or block, samples of up to CAP = 64 / 512 / 2048 / 8192 points with
//   NT = 64 / 256 / 512 / 1024 threads.  The nonzero vectors are compacted into LDS and their half-plane images sorted by
//   angle (plane_sweep.h).  Cuts lie after the last element and wherever two neighbours have cross != 0; for a cut
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
#include "plane_sweep.h"

namespace sd {

constexpr int HX_PT = 256;                                         // pairwise: threads, values of j per workgroup, tile
constexpr double HX_SWEEP_LAUNCH = 17179869184.0;                  // 2^34 comparator evaluations per sweep launch
constexpr double HX_PAIR_LAUNCH = 68719476736.0;                   // 2^36 predicate pairs per pairwise launch
constexpr int HX_NONE = 0x7fffffff;

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
    __shared__ double sx[CAP];
    __shared__ double sy[CAP];
    __shared__ int s_run[CAP / 64];                                 // flags set per run of 64 positions, then their prefix
    __shared__ int s_cnt, s_nz, s_min, s_t1;
    const int t = threadIdx.x, lane = t & 63;
    const i64 q = q0 + blockIdx.x;
    const PointView w = point_view_coop<NT>(sel, P, n, 2, q, &s_cnt);
    const int wcnt = (int)w.cnt;                                    // <= CAP: the launcher chose the tier
    if (t == 0) s_min = HX_NONE;
    const int cnt = hx_compact<NT, false>(P, w, sx, sy, &s_nz);     // the nonzero vectors, in any order
    const int c0 = wcnt - cnt + w.self();
    if (cnt == 0) {                                                 // (block-uniform) also the empty block: 0
        if (t == 0) out[q] = (i64)c0;
        return;
    }
    hx_sort<NT>(sx, sy, cnt);
    // F1(s) = #{i <= s : f}: per run of 64 positions by ballot, the runs by one wave
    const int T1 = hx_flag_prefix<CAP, NT>(sx, sy, cnt, s_run, &s_t1, nullptr);
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
