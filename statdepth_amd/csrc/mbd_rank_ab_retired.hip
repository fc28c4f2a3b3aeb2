// mbd_rank_ab_retired.hip -- the sort-based predecessors of the bucket kernel for n <= 16384 (SD_RANK_IMPL = 3, 2; 1 with
// J >= 4), linked into libstatdepth_hip_xcheck.so only: independent implementations the parity tests compare the product
// path (mbd_rank_ab.hip, mbd_rank_bucket.hip) with.  They write the same u16-pair image the bucket kernel's image mode
// writes; launch_mbd_rank folds it.
//  A  rank_packed_kernel  -- one workgroup sorts one row in LDS (rank_sort.h).  The curve index rides in
//     the low log2(N) mantissa bits of the fp64 key, so v_min_f64 / v_max_f64 sort value and owner
//     together and the holder of sorted position p knows which curve sits there: rank = p, handed to the
//     owner through LDS, written out as (B, A) pairs of uint16.  Exact unless two keys agree above the
//     index field (values within ~2^-38 relative, incl. exact ties): such a row is flagged for kernel B
//     instead, and a workgroup that met one leaves the rest of its rows to kernel B directly.  NaN / +-inf /
//     padding map to sentinel classes beyond every finite class; finite values that would fall into a
//     sentinel class or (non-zero) into the zero class are left to kernel B as well.
//  B  rank_search_kernel  -- the flagged rows: sort of the plain values, then every curve binary-searches
//     its own value (lower bound = B, upper bound gives A; ties are exact by construction).

#include "sd_common.h"
#include "rank_routes.h"
#include "rank_sort.h"

namespace sd {

constexpr u32 ROW_DEFERRED = 0xFFFFFFFFu;    // nnan_out[r]: the packed kernel left row r to the search kernel

template <int NT, int E>
struct PKeys {
    using C = R2Cfg<NT, E>;
    static constexpr int LN = C::LN;
    static constexpr u64 MASK = (u64)C::N - 1;                 // index field
    static constexpr u64 TOPM = ((0xFFFFFFFFFFFFFull >> LN) << LN);
    static constexpr u64 H3 = (0x7FEull << 52) | TOPM;         // padding class (largest)
    static constexpr u64 H2 = H3 - ((u64)1 << LN);             // NaN class
    static constexpr u64 H1 = H3 - ((u64)2 << LN);             // +inf class
    static constexpr u64 SIGN = 0x8000000000000000ull;
    static constexpr u64 LOW = (u64)1 << LN;                   // magnitudes below this share the zero class
};

__device__ __forceinline__ u64 pk_bits(double v) { return (u64)__double_as_longlong(v); }
__device__ __forceinline__ double pk_dbl(u64 b) { return __longlong_as_double((long long)b); }

// ---------------------------------------------------------------------------------------------------
// A: packed keys, rank = position.  Rows [row0, row0 + rows) of Y; AB and nnan are indexed by row - row0.
// ---------------------------------------------------------------------------------------------------
template <int NT, int E>
__global__ __launch_bounds__(NT) void rank_packed_kernel(const double *__restrict__ Y, i64 n64, i64 row0, i64 rows,
                                                         u32 *__restrict__ AB, u32 *__restrict__ nnan_out) {
    using C = R2Cfg<NT, E>;
    using K = PKeys<NT, E>;
    using Sorter = R2Sorter<NT, E>;
    constexpr int LN = C::LN, WB = C::WB;
    constexpr u64 MASK = K::MASK;
    constexpr u64 CLS_NAN = K::H2 >> LN, CLS_PAD = K::H3 >> LN;
    extern __shared__ double Sm[];
    double *firstkey = Sm + C::SLOTS;                          // NT doubles behind the sort image
    __shared__ u32 s_nnan[2];
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int n = (int)n64;
    const int n_act = ((n + WB - 1) / WB) * WB;
    const bool wreal = wave * WB < n_act;
    const double INF = __builtin_huge_val();
    const double MAXK = pk_dbl(K::H3 | MASK);
    if (t < 2) s_nnan[t] = 0;

    const int i0 = wave * WB + lane;                           // loaded curves: i0 + 64 e (512 B per wave instruction)
    double k[E];
    auto load_row = [&](i64 r) {
        const double *rp = Y + (row0 + r) * n + i0;
#pragma unroll
        for (int e = 0; e < E; ++e) k[e] = (i0 + e * 64 < n) ? rp[e * 64] : INF;
    };
    if (wreal && (i64)blockIdx.x < rows) load_row(blockIdx.x);
    __syncthreads();

    int par = 0;
    bool defer = false;                     // after one listed row this workgroup stops trying the packed path
    for (i64 r = blockIdx.x; r < rows; r += gridDim.x) {
        if (defer) {
            if (t == 0) nnan_out[r] = ROW_DEFERRED;
            continue;
        }
        // Per-row opaque copy of the thread id: every LDS address below derives from it, so the compiler
        // recomputes those few ALU ops per row instead of hoisting ~45 loop-invariant address registers out
        // of the row loop and spilling them (measured: 190 B/lane of scratch, +95 MB of HBM traffic per launch).
        int tv = t;
        asm volatile("" : "+v"(tv));
        // ---- pack: value bits above the index field | curve index ----
        int forcefull = 0;
        u32 mynan = 0;
        if (wreal) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int i = i0 + e * 64;
                const u64 b = pk_bits(k[e]);
                const u64 a = b & ~K::SIGN;
                u64 kb = b & ~MASK;
                // one unsigned range test flags zero class, sentinel classes, +-inf and NaN
                if (__builtin_expect((a - K::LOW) >= (K::H1 - K::LOW), 0)) {
                    if (a > 0x7FF0000000000000ull) { kb = K::H2; mynan += (i < n); }
                    else if (a == 0x7FF0000000000000ull) kb = (b & K::SIGN) ? (K::SIGN | K::H3) : K::H1;
                    else if (a == 0) kb = 0;                                   // -0 -> +0
                    else forcefull |= (i < n);         // finite value inside a sentinel / the zero class
                }
                kb = (i < n) ? kb : K::H3;
                k[e] = pk_dbl(kb | (u64)i);
            }
        }
        if (mynan) atomicAdd(&s_nnan[par], mynan);
        Sorter::sort(k, Sm, tv, n_act, wreal, MAXK);

        // ---- any class with several members?  (holders of the sorted positions, layout 0: p = t*E + e) ----
        if (wreal) firstkey[tv] = k[0];
        __syncthreads();
        if (t == 0) s_nnan[par ^ 1] = 0;                       // nobody touches the other parity during this row
        const u32 nnan = s_nnan[par];
        par ^= 1;
        int anytie = 0;
        if (wreal) {
            u64 nextb = ~0ull;
            if ((tv + 1) * E < n_act) nextb = pk_bits(firstkey[tv + 1]);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const u64 c0 = pk_bits(k[e]) >> LN;
                const u64 c1 = ((e < E - 1) ? pk_bits(k[e + 1]) : nextb) >> LN;
                anytie |= (c0 == c1) & (c0 != CLS_NAN) & (c0 != CLS_PAD);
            }
        }
        const int mode = __syncthreads_or(anytie | forcefull);
        const i64 rnext = r + gridDim.x;
        if (mode) {
            if (t == 0) nnan_out[r] = ROW_DEFERRED;
            defer = true;
            continue;
        }
        // ---- ranks are positions: scatter to the owners' slots (the sort image is dead) ----
        const u32 nreal = (u32)n - nnan;                       // non-NaN values occupy sorted positions [0, nreal)
        u32 *R = reinterpret_cast<u32 *>(Sm);
        if (wreal) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const u64 b = pk_bits(k[e]);
                const int idx = (int)(b & MASK);
                const u32 p = (u32)(tv * E + e);
                if (idx < n) R[idx] = ((b >> LN) == CLS_NAN) ? AB_SPECIAL : (p | ((nreal - 1u - p) << 16));
            }
        }
        __syncthreads();
        if (wreal && rnext < rows) load_row(rnext);            // key registers are free: next row in flight
        u32 *dst = AB + r * n + tv;                            // coalesced: curve t + e*NT
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (tv + e * NT < n) dst[e * NT] = R[tv + e * NT];
        if (t == 0) nnan_out[r] = nnan;
        __syncthreads();                                       // LDS is reused by the next row
    }
}

// ---------------------------------------------------------------------------------------------------
// B: plain values + search.  only_deferred == 0: every row of [row0, row0 + rows); otherwise only the rows
// the packed kernel marked ROW_DEFERRED -- workgroup g of this kernel looks at exactly the rows workgroup g
// of the packed kernel owned (same grid), so no list, counter or memset is needed.
// ---------------------------------------------------------------------------------------------------
template <int NT, int E>
__global__ __launch_bounds__(NT) void rank_search_kernel(const double *__restrict__ Y, i64 n64, i64 row0, i64 rows,
                                                         u32 *__restrict__ AB, u32 *__restrict__ nnan_out,
                                                         int only_deferred) {
    using C = R2Cfg<NT, E>;
    using Sorter = R2Sorter<NT, E>;
    constexpr int N = C::N, LE = C::LE, WB = C::WB;
    extern __shared__ double Sm[];
    __shared__ u32 s_nnan[2];
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int n = (int)n64;
    const int n_act = ((n + WB - 1) / WB) * WB;
    const bool wreal = wave * WB < n_act;
    const double INF = __builtin_huge_val();
    if (t < 2) s_nnan[t] = 0;

    const int i0 = wave * WB + lane;
    double k[E];
    auto load_row = [&](i64 r) {
        const double *rp = Y + (row0 + r) * n + i0;
#pragma unroll
        for (int e = 0; e < E; ++e) k[e] = (i0 + e * 64 < n) ? rp[e * 64] : INF;
    };
    __syncthreads();

    int par = 0;
    for (i64 r = blockIdx.x; r < rows; r += gridDim.x) {
        if (only_deferred && nnan_out[r] != ROW_DEFERRED) continue;     // block-uniform
        const double *__restrict__ row = Y + (row0 + r) * n;
        if (wreal) load_row(r);
        int tv = t;                         // per-row opaque copy: keeps LDS addresses out of loop-invariant spills
        asm volatile("" : "+v"(tv));
        // NaN -> +inf, counted (pandas skipna, _containment.py:68-69)
        u32 mynan = 0;
        if (wreal) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                bool isn = k[e] != k[e];
                mynan += isn ? 1u : 0u;
                k[e] = isn ? INF : k[e];
            }
        }
        if (mynan) atomicAdd(&s_nnan[par], mynan);
        Sorter::sort(k, Sm, tv, n_act, wreal, INF);
        if (wreal) {
            double *Sw = Sm + r2_base<0, LE>(tv);
#pragma unroll
            for (int e = 0; e < E; ++e) Sw[r2_off<0, LE>(e)] = k[e];
        }
        __syncthreads();
        if (t == 0) s_nnan[par ^ 1] = 0;    // nobody touches the other parity during this row
        const u32 nnan = s_nnan[par];
        par ^= 1;
        // every wave searches (curve t + e*NT belongs to thread t) although only the waves below n_act
        // sorted: the search is a chain of dependent LDS reads and needs all the parallelism it can get
        {
            const double *xp = row + t;
            u32 *dst = AB + r * n + t;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if ((e & 3) == 0) __builtin_amdgcn_sched_barrier(0);   // at most 4 searches in flight (VGPRs)
                if (t + e * NT < n) {
                    double x = xp[e * NT];
                    u32 ab = AB_SPECIAL;
                    if (x == x) {
                        int lo = r2_bound<N, SlotPad<LE>, false, false>(Sm, n_act, x, INF);   // x is in the row
                        // upper bound: x sits at lo; gallop over its tie run (1 probe if untied, ~2 log2(run) otherwise)
                        int hi = lo + 1, step = 1;
                        while (hi + step <= n_act && Sm[r2_phys<LE>(hi + step - 1)] <= x) { hi += step; step <<= 1; }
                        while (step > 1) {
                            step >>= 1;
                            if (hi + step <= n_act && Sm[r2_phys<LE>(hi + step - 1)] <= x) hi += step;
                        }
                        // keys <= x within [0, n_act) are real non-NaN values unless x = +inf
                        u32 A = (x == INF) ? 0u : (u32)(n - hi) - nnan;
                        ab = (u32)lo | (A << 16);
                    }
                    dst[e * NT] = ab;
                }
            }
        }
        __syncthreads();                    // LDS is reused by the next row; every thread has read the flag
        if (t == 0) nnan_out[r] = nnan;
    }
}

static int ab_grid(i64 rows, int per_cu = 1) {
    const int cus = device_cus() * per_cu;
    return (int)(rows < cus ? rows : cus);
}

template <int NT, int E>
static int launch_sorts(const double *Y, i64 n, i64 row0, i64 rows, u32 *AB, u32 *nnan, int impl, hipStream_t s) {
    using C = R2Cfg<NT, E>;
    // workgroups per CU: limited by LDS (160 KiB) and by 16 waves per CU at up to 128 VGPRs per lane
    constexpr int BY_LDS = (int)(163840 / (C::LDS_BYTES + 512)), BY_WAVES = 1024 / NT;
    constexpr int PER_CU = BY_LDS < BY_WAVES ? (BY_LDS < 1 ? 1 : BY_LDS) : BY_WAVES;
    const int G = ab_grid(rows, PER_CU);
    auto ks = rank_search_kernel<NT, E>;
    SD_HIP(hipFuncSetAttribute((const void *)ks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES));
    if (impl == 2) {   // full keys + search for every row (A/B timing, cross-check)
        hipLaunchKernelGGL(ks, dim3(G), dim3(NT), C::LDS_BYTES, s, Y, n, row0, rows, AB, nnan, 0);
        SD_HIP(hipGetLastError());
        return SD_OK;
    }
    if (impl == 4) {   // the bucket kernel ranked the rows; only those it deferred are sorted here
        hipLaunchKernelGGL(ks, dim3(G), dim3(NT), C::LDS_BYTES, s, Y, n, row0, rows, AB, nnan, 1);
        SD_HIP(hipGetLastError());
        return SD_OK;
    }
    auto kp = rank_packed_kernel<NT, E>;
    const size_t lds = C::LDS_BYTES + (size_t)NT * 8;
    SD_HIP(hipFuncSetAttribute((const void *)kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kp, dim3(G), dim3(NT), lds, s, Y, n, row0, rows, AB, nnan);
    hipLaunchKernelGGL(ks, dim3(G), dim3(NT), C::LDS_BYTES, s, Y, n, row0, rows, AB, nnan, 1);   // same grid!
    SD_HIP(hipGetLastError());
    return SD_OK;
}

int retired_rank_sorts(const double *Y, i64 n, i64 row0, i64 rows, u32 *AB, u32 *nnan, int impl, hipStream_t s) {
    // E = 16 keys per thread throughout; smaller rows take smaller workgroups so that several rows are in
    // flight per CU (n = 4000: 4 workgroups of 256 threads per CU, 0.053 ms against 0.091 ms for 1024 x 4)
    if (n <= 1024) return launch_sorts<64, 16>(Y, n, row0, rows, AB, nnan, impl, s);
    if (n <= 2048) return launch_sorts<128, 16>(Y, n, row0, rows, AB, nnan, impl, s);
    if (n <= 4096) return launch_sorts<256, 16>(Y, n, row0, rows, AB, nnan, impl, s);
    if (n <= 8192) return launch_sorts<512, 16>(Y, n, row0, rows, AB, nnan, impl, s);
    return launch_sorts<1024, 16>(Y, n, row0, rows, AB, nnan, impl, s);
}

}  // namespace sd
