// mbd_rank_big_retired.hip -- the retired generations of the large-n rank route (mbd_rank_big.hip), linked into
// libstatdepth_hip_xcheck.so only: independent implementations the parity tests compare the product path with.
//
// Second generation (SD_BIG_GEN2 = 1; SD_BIG_SORT = 1, SD_BIG_PART1 = 1 pick the first generation's kernel for one step):
// sample-partition into value buckets, so that no rank needs another bucket's keys.
//   S  bucket_splitters_kernel  one workgroup per row sorts a strided sample in LDS and publishes NB-1 splitters
//                               (NB ~ n / 5 500 buckets of capacity 8 192).
//   P  bucket_partition_kernel  (first generation) every element finds its bucket (binary search over the splitters in LDS;
//                               equal values always land together), slots are handed out with one LDS
//                               atomic per element and one global atomic per (workgroup, bucket); values
//                               and curve ids are scattered into the bucket arrays.  NaNs never enter a
//                               bucket: they are counted and marked in the pair image right here.
//   P' bucket_partition2_kernel the same partition with the scatter staged through LDS.
//   A  bucket_packed_kernel     (first generation) one workgroup per (row, bucket): packed-key sort (slot index in the low
//                               mantissa bits, rank_sort.h), rank = bucket base + position, handed to the
//                               slot's owner through LDS and scattered to the curve's pair.  A bucket with
//                               ties or near-ties is flagged for B.
//   A' bucket_rank_kernel       the fp64 bucket ranking without a sort (bucket_rank_item, rank_big_common.h).
//   B  bucket_search_kernel     sort of the plain values + binary search inside a flagged bucket (exact for ties).
// Chunked route (every row with SD_BIG_IMPL = 1; behind the second generation for the rows whose partition overflowed a
//   bucket): a row is cut into chunks of 16 384 keys in curve order: chunk_sort_kernel sorts every chunk,
//   chunk_search_kernel streams every sorted chunk of the row through LDS and sums lower/upper bounds per chunk:
//   O((n/C)^2) chunk searches per row instead of none.  The product runs B and this route as ONE kernel per batch
//   (big_fallback_kernel) and so has no use for the three stand-alone kernels.
#include "rank_big_common.h"
#include "rank_routes.h"

namespace sd {

__global__ __launch_bounds__(BIG_NT) void chunk_sort_kernel(const double *__restrict__ Y, i64 n, i64 row0, i64 rows, i64 nch,
                                                            double *__restrict__ sorted, i64 sstride,
                                                            u32 *__restrict__ nanrow, const u32 *__restrict__ rowflag,
                                                            const u32 *__restrict__ gate, u32 epoch) {
    extern __shared__ double Sm[];
    if (gate && *gate != epoch) return;                       // no row of this batch overflowed its value buckets
    chunk_sort_items(Y, n, row0, rows, nch, sorted, sstride, nanrow, rowflag, Sm);
}

__global__ __launch_bounds__(BIG_NT) void chunk_search_kernel(const double *__restrict__ Y, i64 n, i64 row0,
                                                              i64 rows, const double *__restrict__ sorted,
                                                              i64 sstride, const u32 *__restrict__ nanrow,
                                                              int nchunks, const u32 *__restrict__ rowflag,
                                                              const u32 *__restrict__ gate, u32 epoch, AB2 ab) {
    extern __shared__ double Sm[];
    if (gate && *gate != epoch) return;                       // no row of this batch overflowed its value buckets
    chunk_search_items(Y, n, row0, rows, sorted, sstride, nanrow, nchunks, rowflag, ab, Sm, blockIdx.x, gridDim.x);
}

// S: grid = rows; spl[r][0..NB-2] ascending.  SNT threads sort a strided sample of SE SNT values: 2 048 for up to 24
// value buckets, 4 096 up to 72, 16 384 above (a bucket's fill scatters with 1 / sqrt(samples per bucket); at n = 10^6 the small
// sample overflowed the 8 192-key buckets and sent every row to the chunked route).
template <int SNT, int SE>
__global__ __launch_bounds__(SNT) void bucket_splitters_kernel(const double *__restrict__ Y, i64 n, i64 row0, int NB,
                                                               double *__restrict__ spl) {
    using Cfg = R2Cfg<SNT, SE>;
    constexpr int E = SE, LE = Cfg::LE, SS = SNT * SE;
    extern __shared__ double Sm[];
    const int t = threadIdx.x;
    const i64 rb = blockIdx.x;
    const double *row = Y + (row0 + rb) * n;
    const double INF = __builtin_huge_val();
    double k[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const i64 s = (i64)t * E + e;                       // sample index, any assignment of samples to slots works
        double v = row[(s * n) / SS];
        k[e] = (v == v) ? v : INF;
    }
    R2Sorter<SNT, SE>::sort(k, Sm, t, SS, true, INF);
    double *Sw = Sm + r2_base<0, LE>(t);
#pragma unroll
    for (int e = 0; e < E; ++e) Sw[r2_off<0, LE>(e)] = k[e];
    __syncthreads();
    for (int b = t; b < NB - 1; b += SNT) {
        const int q = (int)(((i64)(b + 1) * SS) / NB);
        spl[rb * (NB - 1) + b] = Sm[r2_phys<LE>(q)];
    }
}

// P: grid = (ceil(n / 16384), rows)
__global__ __launch_bounds__(1024) void bucket_partition_kernel(const double *__restrict__ Y, i64 n, i64 row0, int NB,
                                                                const double *__restrict__ spl,
                                                                u32 *__restrict__ bcnt, u32 *__restrict__ nnanrow,
                                                                u32 *__restrict__ ovf, double *__restrict__ bval,
                                                                u32 *__restrict__ bidx, AB2 ab, int dbg) {
    __shared__ double s_spl[BK_MAXNB];
    __shared__ u32 s_hist[BK_MAXNB];
    __shared__ u32 s_base[BK_MAXNB];
    const int t = threadIdx.x;
    const i64 rb = blockIdx.y;
    const i64 base = (i64)blockIdx.x * 16384;
    for (int b = t; b < NB; b += 1024) {
        if (b < NB - 1) s_spl[b] = spl[rb * (NB - 1) + b];
        s_hist[b] = 0;
    }
    __syncthreads();
    const double *row = Y + (row0 + rb) * n;
    double x[16];
    u32 bk[16], off[16];
    u32 mynan = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const i64 i = base + t + e * 1024;
        x[e] = (i < n) ? row[i] : 0.0;
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const i64 i = base + t + e * 1024;
        bk[e] = 0xFFFFFFFFu;
        if (i < n) {
            if (x[e] == x[e]) {
                // bucket = number of splitters < x (equal values always share a bucket)
                int lo = 0, hi = NB - 1;
                if (dbg) lo = hi = (int)((u32)(e + t) % (u32)NB);     // timing experiment: no search (results invalid)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_spl[mid] < x[e]) lo = mid + 1;
                    else hi = mid;
                }
                bk[e] = (u32)lo;
                off[e] = atomicAdd(&s_hist[lo], 1u);
            } else {
                ++mynan;
                ab_store_nan(ab, (size_t)(rb * n + i));
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) mynan += __shfl_down(mynan, o);
    if ((t & 63) == 0 && mynan) atomicAdd(&nnanrow[rb], mynan);
    __syncthreads();
    for (int b = t; b < NB; b += 1024) s_base[b] = s_hist[b] ? atomicAdd(&bcnt[rb * NB + b], s_hist[b]) : 0u;
    __syncthreads();
    bool over = false;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        if (bk[e] != 0xFFFFFFFFu) {
            const u32 pos = s_base[bk[e]] + off[e];
            if (pos < (u32)BK_C) {
                const size_t slot = ((size_t)rb * NB + bk[e]) * BK_C + pos;
                bval[slot] = x[e];
                bidx[slot] = (u32)(base + t + e * 1024);
            } else {
                over = true;
            }
        }
    }
    if (over) ovf[rb] = 1u;
}

// P' (second generation): the same partition with the scatter staged through LDS.  One workgroup takes 8 192 consecutive curves
// of one row, orders them by value bucket inside LDS (local slot = LDS-atomic offset + local exclusive prefix of the
// workgroup's bucket counts) and copies the ordered block out: consecutive threads write consecutive elements of a
// bucket's run, so the 12-byte records leave as coalesced stores instead of ~19 interleaved partial runs per wave
// instruction.  grid = (ceil(n / 8192), rows).
constexpr int BP2_NT = 1024, BP2_E = 8, BP2_C = BP2_NT * BP2_E;
__global__ __launch_bounds__(BP2_NT) void bucket_partition2_kernel(const double *__restrict__ Y, i64 n, i64 row0, int NB,
                                                                   const double *__restrict__ spl,
                                                                   u32 *__restrict__ bcnt, u32 *__restrict__ nnanrow,
                                                                   u32 *__restrict__ ovf, double *__restrict__ bval,
                                                                   u32 *__restrict__ bidx, AB2 ab) {
    extern __shared__ double Sm2[];
    double *Skey = Sm2;                                               // [BP2_C]
    u32 *Sid = reinterpret_cast<u32 *>(Skey + BP2_C);                 // [BP2_C]
    unsigned short *Sbk = reinterpret_cast<unsigned short *>(Sid + BP2_C);   // [BP2_C]
    __shared__ double s_spl[BK_MAXNB];
    __shared__ u32 s_hist[BK_MAXNB];
    __shared__ u32 s_gbase[BK_MAXNB];
    __shared__ u32 s_lbase[BK_MAXNB + 1];
    __shared__ u32 s_wtot[BP2_NT / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const i64 rb = blockIdx.y;
    const i64 base = (i64)blockIdx.x * BP2_C;
    for (int b = t; b < BK_MAXNB; b += BP2_NT) {
        if (b < NB - 1) s_spl[b] = spl[rb * (NB - 1) + b];
        s_hist[b] = 0;
    }
    __syncthreads();
    const double *row = Y + (row0 + rb) * n;
    double x[BP2_E];
    u32 bk[BP2_E], off[BP2_E];
    u32 mynan = 0;
#pragma unroll
    for (int e = 0; e < BP2_E; ++e) {
        const i64 i = base + t + e * BP2_NT;
        x[e] = (i < n) ? row[i] : 0.0;
    }
#pragma unroll
    for (int e = 0; e < BP2_E; ++e) {
        const i64 i = base + t + e * BP2_NT;
        bk[e] = 0xFFFFFFFFu;
        off[e] = 0;
        if (i < n) {
            if (x[e] == x[e]) {
                int lo = 0, hi = NB - 1;                    // bucket = number of splitters < x (equal values share a bucket)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_spl[mid] < x[e]) lo = mid + 1;
                    else hi = mid;
                }
                bk[e] = (u32)lo;
                off[e] = atomicAdd(&s_hist[lo], 1u);
            } else {
                ++mynan;
                ab_store_nan(ab, (size_t)(rb * n + i));
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) mynan += __shfl_down(mynan, o);
    if (lane == 0 && mynan) atomicAdd(&nnanrow[rb], mynan);
    __syncthreads();
    // global base of this workgroup's run in every bucket; local exclusive prefix of the counts (one thread per bucket)
    {
        const u32 c = (t < NB) ? s_hist[t] : 0u;
        if (t < NB) s_gbase[t] = c ? atomicAdd(&bcnt[rb * NB + t], c) : 0u;
        const u32 incl = rb_wave_incl_scan(c);
        if (lane == 63) s_wtot[wave] = incl;
        __syncthreads();
        const u32 wt = (lane < BP2_NT / 64) ? s_wtot[lane] : 0u;
        const u32 wscan = rb_row_incl_scan(wt);
        const u32 woff = wave ? rb_readlane(wscan, wave - 1) : 0u;
        if (t < NB) s_lbase[t] = woff + incl - c;
        if (t == BP2_NT - 1) s_lbase[NB] = woff + incl;             // number of non-NaN keys of the block (NB <= 1024)
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < BP2_E; ++e) {
        if (bk[e] != 0xFFFFFFFFu) {
            const u32 lp = s_lbase[bk[e]] + off[e];
            Skey[lp] = x[e];
            Sid[lp] = (u32)(base + t + e * BP2_NT);
            Sbk[lp] = (unsigned short)bk[e];
        }
    }
    __syncthreads();
    const u32 nval = s_lbase[NB];
    bool over = false;
    for (u32 p = t; p < nval; p += BP2_NT) {
        const u32 b = Sbk[p];
        const u32 g = s_gbase[b] + (p - s_lbase[b]);
        if (g < (u32)BK_C) {
            const size_t slot = ((size_t)rb * NB + b) * BK_C + g;
            bval[slot] = Skey[p];
            bidx[slot] = Sid[p];
        } else {
            over = true;
        }
    }
    if (over) ovf[rb] = 1u;
}

template <int NT, int E>
struct BkKeys {
    using C = R2Cfg<NT, E>;
    static constexpr int LN = C::LN;
    static constexpr u64 MASK = (u64)C::N - 1;
    static constexpr u64 TOPM = ((0xFFFFFFFFFFFFFull >> LN) << LN);
    static constexpr u64 H3 = (0x7FEull << 52) | TOPM;         // padding class (largest)
    static constexpr u64 H1 = H3 - ((u64)2 << LN);             // +inf class (H3 - 1 class stays unused here: no NaN)
    static constexpr u64 SIGN = 0x8000000000000000ull;
    static constexpr u64 LOW = (u64)1 << LN;
};

__device__ __forceinline__ u64 bk_bits(double v) { return (u64)__double_as_longlong(v); }
__device__ __forceinline__ double bk_dbl(u64 b) { return __longlong_as_double((long long)b); }

// A: grid = (NB, rows)
__global__ __launch_bounds__(BK_NT) void bucket_packed_kernel(i64 n, int NB, const u32 *__restrict__ bcnt,
                                                              const u32 *__restrict__ nnanrow,
                                                              const u32 *__restrict__ ovf,
                                                              const double *__restrict__ bval,
                                                              const u32 *__restrict__ bidx, u32 *__restrict__ bflag,
                                                              AB2 ab) {
    using C = BkCfg;
    using K = BkKeys<BK_NT, BK_E>;
    constexpr int E = BK_E, NT = BK_NT, LN = C::LN, WB = C::WB;
    constexpr u64 MASK = K::MASK, CLS_PAD = K::H3 >> LN;
    extern __shared__ double Sm[];
    double *firstkey = Sm + C::SLOTS;
    __shared__ u32 s_basecnt;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x;
    const i64 rb = blockIdx.y;
    if (ovf[rb]) return;
    const int cnt = (int)bcnt[rb * NB + b];
    if (cnt == 0) return;
    if (t == 0) {
        u32 s = 0;
        for (int q = 0; q < b; ++q) s += bcnt[rb * NB + q];
        s_basecnt = s;
    }
    const int n_act = ((cnt + WB - 1) / WB) * WB;
    const bool wreal = wave * WB < n_act;
    const double INF = __builtin_huge_val();
    const double MAXK = bk_dbl(K::H3 | MASK);
    const size_t slot0 = ((size_t)rb * NB + b) * BK_C;
    const int i0 = wave * WB + lane;
    double k[E];
    int forcefull = 0;
    if (wreal) {
        const double *rp = bval + slot0 + i0;
#pragma unroll
        for (int e = 0; e < E; ++e) k[e] = (i0 + e * 64 < cnt) ? rp[e * 64] : INF;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int j = i0 + e * 64;
            const u64 bits = bk_bits(k[e]);
            const u64 a = bits & ~K::SIGN;
            u64 kb = bits & ~MASK;
            if (__builtin_expect((a - K::LOW) >= (K::H1 - K::LOW), 0)) {
                if (a == 0x7FF0000000000000ull) kb = (bits & K::SIGN) ? (K::SIGN | K::H3) : K::H1;
                else if (a == 0) kb = 0;
                else forcefull |= (j < cnt);
            }
            kb = (j < cnt) ? kb : K::H3;
            k[e] = bk_dbl(kb | (u64)j);
        }
    }
    R2Sorter<NT, E>::sort(k, Sm, t, n_act, wreal, MAXK);
    if (wreal) firstkey[t] = k[0];
    __syncthreads();
    int anytie = 0;
    if (wreal) {
        u64 nextb = ~0ull;
        if ((t + 1) * E < n_act) nextb = bk_bits(firstkey[t + 1]);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const u64 c0 = bk_bits(k[e]) >> LN;
            const u64 c1 = ((e < E - 1) ? bk_bits(k[e + 1]) : nextb) >> LN;
            anytie |= (c0 == c1) & (c0 != CLS_PAD);
        }
    }
    if (__syncthreads_or(anytie | forcefull)) {
        if (t == 0) bflag[rb * NB + b] = 1u;
        return;
    }
    u32 *R = reinterpret_cast<u32 *>(Sm);
    if (wreal) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int j = (int)(bk_bits(k[e]) & MASK);
            if (j < cnt) R[j] = (u32)(t * E + e);
        }
    }
    __syncthreads();
    const u32 base = s_basecnt;
    for (int j = t; j < cnt; j += NT) {
        ab.B[rb * n + bidx[slot0 + j]] = base + R[j];               // distinct keys: A = (n - NaNs of the row) - 1 - B
    }
}

// A' as a kernel of its own: grid = 8 * NB * ceil(rows / 8), every row
__global__ __launch_bounds__(BR_NT) void bucket_rank_kernel(i64 n, i64 rows, int NB, const u32 *__restrict__ bcnt,
                                                            const u32 *__restrict__ nnanrow,
                                                            const u32 *__restrict__ ovf,
                                                            const double *__restrict__ bval,
                                                            const u32 *__restrict__ bidx, u32 *__restrict__ bflag,
                                                            AB2 ab) {
    bucket_rank_item(blockIdx.x, n, rows, NB, bcnt, nnanrow, ovf, nullptr, bval, bidx, bflag, nullptr, 0u, ab);
}

__global__ __launch_bounds__(BK_NT) void bucket_search_kernel(const double *__restrict__ Y, i64 n, i64 row0, i64 rows, int NB,
                                                              const u32 *__restrict__ bcnt,
                                                              const u32 *__restrict__ nnanrow,
                                                              const u32 *__restrict__ bflag,
                                                              const u32 *__restrict__ rowtied,
                                                              const double *__restrict__ bval,
                                                              const u32 *__restrict__ bidx,
                                                              const u32 *__restrict__ gate, u32 epoch, AB2 ab) {
    extern __shared__ double Sm[];
    if (gate && *gate != epoch) return;                               // no bucket of this batch was flagged
    bucket_search_items<BK_NT, BK_E>(Y, n, row0, rows, NB, bcnt, nnanrow, bflag, rowtied, bval, bidx, ab, Sm);
}

// Ranks one batch the retired way.  SD_BIG_IMPL = 1: the chunked route for every row; else the second generation
// (S -> P' or P -> A' or the packed-key sort -> B) and the chunked route for the rows whose partition overflowed.
// *nnan_rows: where the rows' NaN counts are for the fold.
int retired_big_rank_batch(const BigBatch &b, hipStream_t s, const u32 **nnan_rows) {
    const bool buckets = xswitch("SD_BIG_IMPL") != 1;
    const int NB = b.NB;
    const i64 n = b.n, row0 = b.row0, rows = b.rows;
    const int cus = device_cus();
    const unsigned pgrid = (unsigned)cus;                   // small persistent grids of the fallback kernels
    auto k_cs = chunk_sort_kernel;
    auto k_cq = chunk_search_kernel;
    auto k_bs = bucket_search_kernel;
    auto k_br = bucket_rank_kernel;
    auto k_bp = bucket_packed_kernel;
    auto k_sp_small = bucket_splitters_kernel<128, 16>;
    auto k_sp = bucket_splitters_kernel<256, 16>;
    auto k_sp_big = bucket_splitters_kernel<1024, 16>;
    constexpr size_t lds_sp_small = R2Cfg<128, 16>::LDS_BYTES, lds_sp = R2Cfg<256, 16>::LDS_BYTES;
    constexpr size_t lds_sp_big = R2Cfg<1024, 16>::LDS_BYTES;
    const size_t lds_bk = BkCfg::LDS_BYTES + (size_t)BK_NT * 8;
    SD_HIP(hipFuncSetAttribute((const void *)k_cs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BigCfg::LDS_BYTES));
    SD_HIP(hipFuncSetAttribute((const void *)k_cq, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BigCfg::LDS_BYTES));
    SD_HIP(hipFuncSetAttribute((const void *)k_bs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BkCfg::LDS_BYTES));
    SD_HIP(hipFuncSetAttribute((const void *)k_br, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BR_LDS));
    SD_HIP(hipFuncSetAttribute((const void *)k_sp_small, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sp_small));
    SD_HIP(hipFuncSetAttribute((const void *)k_sp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sp));
    SD_HIP(hipFuncSetAttribute((const void *)k_sp_big, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sp_big));
    SD_HIP(hipFuncSetAttribute((const void *)k_bp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bk));
    SD_HIP(hipFuncSetAttribute((const void *)bucket_partition2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)((size_t)BP2_C * 14)));

    const u32 *fallback_rows = nullptr;                      // chunked route: every row
    *nnan_rows = b.nanf;
    SD_HIP(hipMemsetAsync(b.zero, 0, b.zero_bytes, s));
    if (buckets) {
        const bool rank_nosort = xswitch("SD_BIG_SORT") != 1;
        if (NB <= 24)
            hipLaunchKernelGGL(k_sp_small, dim3((unsigned)rows), dim3(128), lds_sp_small, s, b.Y, n, row0, NB, b.spl);
        else if (NB <= 72)
            hipLaunchKernelGGL(k_sp, dim3((unsigned)rows), dim3(256), lds_sp, s, b.Y, n, row0, NB, b.spl);
        else
            hipLaunchKernelGGL(k_sp_big, dim3((unsigned)rows), dim3(1024), lds_sp_big, s, b.Y, n, row0, NB, b.spl);
        if (xswitch("SD_BIG_PART1") == 1)                    // first-generation partition (direct scatter)
            hipLaunchKernelGGL(bucket_partition_kernel, dim3((unsigned)((n + 16383) / 16384), (unsigned)rows), dim3(1024),
                               0, s, b.Y, n, row0, NB, (const double *)b.spl, b.bcnt, b.nnanrow, b.ovf, b.bval, b.bidx, b.ab, 0);
        else
            hipLaunchKernelGGL(bucket_partition2_kernel, dim3((unsigned)((n + BP2_C - 1) / BP2_C), (unsigned)rows),
                               dim3(BP2_NT), (size_t)BP2_C * 14, s, b.Y, n, row0, NB, (const double *)b.spl, b.bcnt, b.nnanrow,
                               b.ovf, b.bval, b.bidx, b.ab);
        if (!rank_nosort)
            hipLaunchKernelGGL(k_bp, dim3((unsigned)NB, (unsigned)rows), dim3(BK_NT), lds_bk, s, n, NB, (const u32 *)b.bcnt,
                               (const u32 *)b.nnanrow, (const u32 *)b.ovf, (const double *)b.bval, (const u32 *)b.bidx, b.bflag,
                               b.ab);
        else
            hipLaunchKernelGGL(k_br, dim3((unsigned)(8 * NB * ((rows + 7) / 8))), dim3(BR_NT), BR_LDS, s, n, rows, NB,
                               (const u32 *)b.bcnt, (const u32 *)b.nnanrow, (const u32 *)b.ovf,
                               (const double *)b.bval, (const u32 *)b.bidx, b.bflag, b.ab);
        hipLaunchKernelGGL(k_bs, dim3(pgrid), dim3(BK_NT), BkCfg::LDS_BYTES, s, b.Y, n, row0, rows, NB, (const u32 *)b.bcnt,
                           (const u32 *)b.nnanrow, (const u32 *)b.bflag, (const u32 *)nullptr, (const double *)b.bval,
                           (const u32 *)b.bidx, (const u32 *)nullptr, 0u, b.ab);
        fallback_rows = b.ovf;
        *nnan_rows = b.nnanrow;
    }
    // no gate: the chunk kernels look at every row flag
    const unsigned csgrid = fallback_rows ? pgrid : (unsigned)(b.nch * rows < 65535 * 16 ? b.nch * rows : 65535 * 16);
    hipLaunchKernelGGL(k_cs, dim3(csgrid), dim3(BIG_NT), BigCfg::LDS_BYTES, s, b.Y, n, row0, rows, b.nch,
                       b.sorted, b.sstride, b.nanf, fallback_rows, (const u32 *)nullptr, 0u);
    i64 rgroups = cus / b.nch;
    if (rgroups < 1) rgroups = 1;
    if (rgroups > rows) rgroups = rows;
    hipLaunchKernelGGL(k_cq, dim3((unsigned)(rgroups * b.nch)), dim3(BIG_NT), BigCfg::LDS_BYTES, s, b.Y, n, row0, rows,
                       (const double *)b.sorted, b.sstride, (const u32 *)b.nanf, (int)b.nch, fallback_rows,
                       (const u32 *)nullptr, 0u, b.ab);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

}  // namespace sd
