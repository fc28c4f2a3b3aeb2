// bd_strict_subsets.hip -- K3 strict band depth (relax=False, J = 2) inside EXPLICIT blocks of curves: the K-block sampled
// estimator's (subset, target) pairs, one workgroup per pair, masks in LDS (or in a slice of the workspace for large blocks).
// Independent of the mask / matching pipeline of bd_strict.hip; sd_api.hip calls the three functions declared in sd_common.h.
#include "sd_common.h"

namespace sd {

// ---------------------------------------------------------------------------------------------------
// Strict band depth (J = 2) of one target inside an explicit subset of the curves, for nb (subset, target) pairs in one
// launch: the K-block sampled estimator with the reference's default relax=False (_samplefunctionaldepth,
// _functional.py:170-182 calls _univariate_band_depth on n*K small blocks).  One workgroup per pair: the block's masks
// against its target are built in LDS (u32[members][2 W32 + 1], the + 1 keeps rows on different banks), then every
// thread walks the pairs (a, b > a) of its members a with an early exit per four words.  Blocks are small (n / K
// curves), so the whole pair fits the LDS: members * (2 W32 + 1) * 4 + bs * 4 bytes; larger ones keep their masks in a
// slice of the workspace instead (the kernel's scratch argument; refused only when bs * 4 + 64 exceeds the LDS).
// ---------------------------------------------------------------------------------------------------
constexpr int ST_SUB_THREADS = 512;
constexpr int ST_SUB_GRID = 2048;                               // workgroups (and scratch slices) of the large-block form
static inline size_t strict_subset_lds(i64 T, int bs) { return (size_t)bs * (2 * ((T + 31) / 32) + 1) * 4 + (size_t)bs * 4 + 64; }
bool bd_strict_subsets_supported(i64 T, int bs) { return strict_subset_lds(T, bs) <= 160 * 1024 - 2048; }
// blocks whose masks do not fit the LDS keep them in a slice of the workspace (L2-resident: a slice is read bs times)
size_t bd_strict_subsets_workspace_bytes(i64 T, i64 nb, int bs) {
    if (bd_strict_subsets_supported(T, bs)) return 0;
    const i64 g = nb < ST_SUB_GRID ? nb : ST_SUB_GRID;
    return (size_t)g * bs * (2 * ((T + 31) / 32) + 1) * 4 + 256;
}

// grid-stride over the (subset, target) pairs; scratch == nullptr: masks in LDS
__global__ __launch_bounds__(ST_SUB_THREADS) void strict_subset_kernel(const double *__restrict__ Y, i64 T, i64 n,
                                                                      const int *__restrict__ members, i64 nb, int bs,
                                                                      const int *__restrict__ target, u32 *__restrict__ scratch,
                                                                      u64 *__restrict__ out) {
    extern __shared__ u32 sm[];
    __shared__ u64 red[ST_SUB_THREADS / 64];
    __shared__ int s_cnt;
    const int W32 = (int)((T + 31) / 32);
    const int RW = 2 * W32 + 1;
    int *ids = reinterpret_cast<int *>(sm);                     // [bs] the block's other members
    u32 *mk = scratch ? scratch + (size_t)blockIdx.x * bs * RW : sm + bs;     // [cnt][RW]
    const int tid = threadIdx.x;
    for (i64 k = blockIdx.x; k < nb; k += gridDim.x) {
        __syncthreads();                                        // the previous pair's ids / masks / sums are done with
        const int tg = target[k];
        if (tid == 0) {
            int c = 0;
            for (int e = 0; e < bs; ++e) {
                const int col = members[k * bs + e];
                if (col >= 0 && col != tg) ids[c++] = col;
            }
            s_cnt = c;
        }
        bool tnan = false;
        for (i64 t = tid; t < T; t += ST_SUB_THREADS) {
            const double q = Y[t * n + tg];
            tnan |= q != q;
        }
        const bool anynan = __syncthreads_or(tnan) != 0;        // also publishes ids / s_cnt
        if (anynan) {                                           // NaN in the target: nothing is contained
            if (tid == 0) out[k] = 0;
            continue;
        }
        const int cnt = s_cnt;
        for (int e = tid; e < cnt * W32; e += ST_SUB_THREADS) {
            const int c = e / W32, w = e % W32;
            const i64 col = ids[c];
            u32 un = 0, dn = 0;
            const i64 t0 = (i64)w * 32;
            const int tl = (int)(T - t0 < 32 ? T - t0 : 32);
            for (int t = 0; t < tl; ++t) {
                const double x = Y[(t0 + t) * n + col], q = Y[(t0 + t) * n + tg];
                const bool isn = x != x;
                un |= (x > q || isn) ? (1u << t) : 0u;
                dn |= (x < q || isn) ? (1u << t) : 0u;
            }
            mk[c * RW + w] = un;
            mk[c * RW + W32 + w] = dn;
        }
        __syncthreads();                                        // (global stores of this workgroup are visible to it after the barrier)
        u64 good = 0;
        for (int a = tid; a < cnt; a += ST_SUB_THREADS) {
            const u32 *ra = mk + (size_t)a * RW;
            for (int b = a + 1; b < cnt; ++b) {
                const u32 *rb = mk + (size_t)b * RW;
                u32 bad = 0;
                for (int w = 0; w < W32 && !bad; w += 4) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (w + j < W32) bad |= (ra[w + j] & rb[w + j]) | (ra[W32 + w + j] & rb[W32 + w + j]);
                }
                good += bad == 0;
            }
        }
        for (int o = 32; o > 0; o >>= 1) good += __shfl_down(good, o);
        if ((tid & 63) == 0) red[tid >> 6] = good;
        __syncthreads();
        if (tid == 0) {
            u64 tot = 0;
            for (int j = 0; j < ST_SUB_THREADS / 64; ++j) tot += red[j];
            out[k] = tot;
        }
    }
}

int launch_bd_strict_subsets(const double *Y, i64 T, i64 n, const int *members, i64 nb, int bs, const int *target, u64 *out,
                             void *ws, size_t ws_bytes, hipStream_t s) {
    const bool in_lds = bd_strict_subsets_supported(T, bs);
    if ((size_t)bs * 4 + 64 > 160 * 1024 - 2048)
        return fail(SD_ERR_UNSUPPORTED, "strict subset depth: blocks of %d curves (the member list alone exceeds the LDS)", bs);
    u32 *scratch = nullptr;
    if (!in_lds) {
        const size_t need = bd_strict_subsets_workspace_bytes(T, nb, bs);
        if (!ws || ws_bytes < need)
            return fail(SD_ERR_WORKSPACE, "strict subset depth: %zu bytes of workspace for blocks of %d curves x %lld timepoints "
                        "(sd_bd_strict_subset_workspace_bytes)", need, bs, (long long)T);
        scratch = (u32 *)(((size_t)ws + 255) / 256 * 256);
    }
    const size_t lds = in_lds ? strict_subset_lds(T, bs) : (size_t)bs * 4 + 64;
    SD_HIP(hipFuncSetAttribute((const void *)strict_subset_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const i64 g = in_lds ? (nb < 65535 * 16 ? nb : 65535 * 16) : (nb < ST_SUB_GRID ? nb : ST_SUB_GRID);
    hipLaunchKernelGGL(strict_subset_kernel, dim3((unsigned)g), dim3(ST_SUB_THREADS), lds, s, Y, T, n, members, nb, bs, target, scratch,
                       out);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

}  // namespace sd
