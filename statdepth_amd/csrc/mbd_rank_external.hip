// mbd_rank_external.hip -- X: band totals of EXTERNAL curves (targets that are not members of the set; the homogeneity
// coefficients' `FunctionalDepth(F u {g}, to_compute=[g])`, homogeneity.py:101-128) through the bucket structure of
// rank_bucket_kernel (mbd_rank_bucket.hip), n <= 16384, J <= 3.
//
// Per row the set is histogrammed, prefix-summed and scattered (RbRow, rank_bucket_row.h); then every external value x looks
// up its own bucket -- b(x) is monotone, so the keys of earlier buckets are below x and those of later ones above --
// and compares itself with that bucket's members: B = base + #(y < x), A = n_valid - base - #(y <= x).  O(n + m)
// per row instead of the pairwise kernel's O(n m).  No row is set aside: a row the map cannot spread (equal values,
// an infinity) simply lands in one bucket, and m targets walking n keys is still cheap.
// Thread t owns targets t, t + 1024, ... (EQ of them) and their totals for the whole launch.
#include "sd_common.h"
#include "rank_routes.h"
#include "rank_bucket_row.h"

namespace sd {

template <int NT, int E, int LNB, int J, int EQ>
__global__ __launch_bounds__(NT) void rank_external_kernel(const double *__restrict__ Y, i64 n64, i64 rows,
                                                           const double *__restrict__ Q, i64 m64, i64 qstride,
                                                           u64 *__restrict__ partial) {
    using Row = RbRow<NT, E, LNB, 5, false>;                          // a bucket of 32 keys or more: ties or a wide range?
    extern __shared__ double Sm[];
    const int n = (int)n64, m = (int)m64;
    const int t0 = threadIdx.x;
    const double QNAN = __builtin_nan("");
    const int DUMMY = Row::C::dummy_pos(n);
    int t = t0;
    Row row(Sm);
    double k[E];
    auto load_row = [&](i64 r) {
        const double *rp = Y + r * n + t;
#pragma unroll
        for (int e = 0; e < E; ++e) k[e] = (e < E - 1 || t + (E - 1) * NT < n) ? rp[e * NT] : QNAN;
    };
    u64 acc[EQ][JMAX - 1];
#pragma unroll
    for (int q = 0; q < EQ; ++q)
#pragma unroll
        for (int j = 0; j < JMAX - 1; ++j) acc[q][j] = 0;
    if ((i64)blockIdx.x < rows) load_row(blockIdx.x);
    for (i64 r = blockIdx.x; r < rows; r += gridDim.x) {
        const i64 rnext = r + gridDim.x;
        t = t0;
        asm volatile("" : "+v"(t));                                   // per-row opaque thread id (see rank_bucket_kernel)
        row.thread(t);
        // the row's external values (in flight under the set's phases)
        double xq[EQ];
#pragma unroll
        for (int q = 0; q < EQ; ++q) xq[q] = (t + q * NT < m) ? Q[r * qstride + t + q * NT] : QNAN;
        const typename Row::Built built = row.build(k, n, DUMMY);     // (0) - (3), barriers 1 - 4
        const u32 nv = built.nv, nn = (u32)n - nv;
        if (rnext < rows) load_row(rnext);
        __syncthreads();                                              // barrier 5
        // ---- (4x) every external value against the members of its bucket ----
#pragma unroll
        for (int q = 0; q < EQ; ++q) {
            const double x = xq[q];
            if (x == x) {                                             // NaN target (and target slots beyond m): nothing
                const u32 b = built.bucket_of(x);
                const u32 base = row.H16[b], end = row.H16[b + 1];
                u32 less = 0, le = 0;
                // a value outside the set's range sits in an end bucket and still compares correctly
#pragma unroll 1
                for (u32 j = base; j < end; ++j) {
                    const double y = row.S[j];
                    less += (y < x) ? 1u : 0u;
                    le += (y <= x) ? 1u : 0u;
                }
                band_counts_add<J>(nv - base - le, base + less, nn, (u64)n, acc[q]);
            }
        }
        __syncthreads();                                              // barrier 6: S and the bases have been read
        row.clear();
    }
    t = t0;
    u64 *P = partial + (size_t)blockIdx.x * (J - 1) * m;
#pragma unroll
    for (int q = 0; q < EQ; ++q)
        if (t + q * NT < m) {
#pragma unroll
            for (int j = 0; j < J - 1; ++j) P[(size_t)j * m + t + q * NT] = acc[q][j];
        }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
bool mbd_rank_external_supported(i64 T, i64 n, i64 m, int J) {
    (void)T;
    return n >= 2 && n <= 16384 && J >= 2 && J <= 3 && m >= 1;
}

size_t mbd_rank_external_workspace_bytes(i64 T, i64 n, i64 m, int J) {
    if (!mbd_rank_external_supported(T, n, m, J)) return 0;
    const i64 mc = m < 8192 ? m : 8192;
    return align_up((size_t)device_cus() * (J - 1) * mc * 8, 256) + 512;
}

template <int E, int J>
static int launch_external_cfg(const double *Y, i64 n, i64 rows, const double *Q, i64 m, i64 qstride, u64 *partial, int G,
                               hipStream_t s) {
    constexpr int LNB = rb_lnb(E, 3);
    const size_t lds = RBCfg<1024, E, LNB, 3>::lds_bytes((int)n);
    if (lds > 163840) return fail(SD_ERR_UNSUPPORTED, "external kernel: %zu bytes of LDS for n=%lld", lds, (long long)n);
#define RB_XL(EQ_) return rb_launch(rank_external_kernel<1024, E, LNB, J, EQ_>, G, 1024, lds, s, Y, n, rows, Q, m, qstride, partial);
    if (m <= 1024) RB_XL(1) else if (m <= 2048) RB_XL(2) else if (m <= 4096) RB_XL(4) else RB_XL(8)
#undef RB_XL
}

// Q: T x m time-major; out[q][j] = totals.  Targets go in groups of 8 192 (8 per thread).
int launch_mbd_external_rank(const double *Y, i64 T, i64 n, const double *Q, i64 m, int J, u64 *out, void *ws,
                             size_t ws_bytes, hipStream_t s) {
    if (!mbd_rank_external_supported(T, n, m, J)) return fail(SD_ERR_UNSUPPORTED, "external rank kernel: unsupported shape");
    if (!ws || ws_bytes < mbd_rank_external_workspace_bytes(T, n, m, J))
        return fail(SD_ERR_WORKSPACE, "external rank workspace too small");
    u64 *partial = (u64 *)(((size_t)ws + 255) / 256 * 256);
    const int cus = device_cus();
    const int G = (int)(T < cus ? T : cus);
    const int E = (int)((n + 1023) / 1024);
    for (i64 q0 = 0; q0 < m; q0 += 8192) {
        const i64 mc = m - q0 < 8192 ? m - q0 : 8192;
        int rc = SD_OK;
#define RB_XE(E_) case E_: rc = (J == 2) ? launch_external_cfg<E_, 2>(Y, n, T, Q + q0, mc, m, partial, G, s) \
                                         : launch_external_cfg<E_, 3>(Y, n, T, Q + q0, mc, m, partial, G, s); break;
        switch (E) {
            RB_XE(1) RB_XE(2) RB_XE(3) RB_XE(4) RB_XE(5) RB_XE(6) RB_XE(7) RB_XE(8)
            RB_XE(9) RB_XE(10) RB_XE(11) RB_XE(12) RB_XE(13) RB_XE(14) RB_XE(15) RB_XE(16)
            default: return fail(SD_ERR_UNSUPPORTED, "external rank kernel covers n <= 16384");
        }
#undef RB_XE
        if (rc) return rc;
        if ((rc = launch_rank_finalize(partial, G, 0, nullptr, nullptr, nullptr, T, mc, nullptr, 0, mc, J,
                                       out + q0 * (J - 1), 1, s)))
            return rc;
    }
    return SD_OK;
}

}  // namespace sd
