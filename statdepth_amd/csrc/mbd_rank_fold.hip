// mbd_rank_fold.hip -- K1+K2 rank formulation: the kernels that fold a pair image into the int64 totals of the requested
// targets, C(v,j) - C(A,j) - C(B,j) summed over the rows, and the two entry points that choose among them (rank_routes.h):
//   fold_pair_image  the 16-bit image B | A << 16 of n <= 40 960 (mbd_rank_ab.hip: the bucket kernel's image mode, the medium
//                    route, the retired sort generations): rank_accumulate_kernel, rank_accumulate4_kernel;
//   fold_ab2_image   the AB2 image of the large-n route (mbd_rank_big.hip, rank_big_common.h): rank_accumulate2_kernel,
//                    rank_accumulate2x4_kernel, rank_accumulate_h8_kernel.
// Every kernel is the skeleton of rank_fold.h -- row loop, reduction over the slices, =|+= store, pair decode -- with its own
// load (one word, four through 16 bytes, eight half words through 16 bytes) and its own block shape; rank_accumulate4_kernel
// takes the reduction and store only (see there).

#include "rank_fold.h"

namespace sd {

// ---------------------------------------------------------------------------------------------------
// 16-bit image: out[q][j] (=|+=) sum over the batch's rows of the band counts of target q.
// block = 64 targets x 16 row slices, 8 independent loads in flight per thread: a pure stream over the pair image.
// ---------------------------------------------------------------------------------------------------
template <int J>
__global__ __launch_bounds__(1024) void rank_accumulate_kernel(const u32 *__restrict__ AB, const u32 *__restrict__ nnan,
                                                               i64 rows, i64 n, const i64 *__restrict__ targets,
                                                               i64 tbegin, i64 m, u64 *__restrict__ out, int first) {
    __shared__ u64 red[16][64];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const i64 q = (i64)blockIdx.x * 64 + x;
    const i64 i = (q < m) ? (targets ? targets[q] : tbegin + q) : 0;
    u64 acc[JMAX - 1];
#pragma unroll
    for (int j = 0; j < JMAX - 1; ++j) acc[j] = 0;
    if (q < m)
        fold_rows<16, 8>(
            rows, y, [&](i64 r) { return FoldLoad<u32>{AB[r * n + i], nnan[r]}; },
            [&](const FoldLoad<u32> &v, i64) { fold_pair16<J>(v.w, v.nn, n, acc); });
#pragma unroll
    for (int j = 0; j < J - 1; ++j) fold_store(red, x, y, acc[j], q < m, out + q * (J - 1) + j, first);
}

// Same fold for a contiguous, 4-aligned target block: 16-byte loads (4 curves per lane, 1 KiB per wave
// instruction instead of 256 B).  block = 16 curve quads x 64 row slices.
// The one kernel here with its row loop and its decode written out: behind fold_rows the compiler keeps the row's C(v, j)
// for the four curves and J = 3 drops from 6 waves per SIMD to 5 (74 -> 88 VGPRs); behind fold_pair16 alone J = 7 spills 48
// bytes instead of 32 ("The fold skeleton").
template <int J>
__global__ __launch_bounds__(1024) void rank_accumulate4_kernel(const u32 *__restrict__ AB, const u32 *__restrict__ nnan,
                                                                i64 rows, i64 n, i64 tbegin, i64 m,
                                                                u64 *__restrict__ out, int first) {
    __shared__ u64 red[64][65];
    const int x = threadIdx.x & 15, y = threadIdx.x >> 4;            // quad within block, row slice
    const i64 q4 = ((i64)blockIdx.x * 16 + x) * 4;                   // first of this thread's 4 targets
    u64 acc[4][JMAX - 1];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < JMAX - 1; ++j) acc[c][j] = 0;
    if (q4 < m) {
        const u32 *src = AB + tbegin + q4;
        i64 r = y;
        for (; r + 64 * 3 < rows; r += 64 * 4) {
            uint4 v[4];
            u32 nn[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = *reinterpret_cast<const uint4 *>(src + (r + 64 * u) * n);
                nn[u] = nnan[r + 64 * u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const u32 ab[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (ab[c] != AB_SPECIAL) band_counts_add<J>(ab[c] >> 16, ab[c] & 0xFFFFu, nn[u], (u64)(n - 1), acc[c]);
            }
        }
        for (; r < rows; r += 64) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + r * n);
            const u32 nn = nnan[r];
            const u32 ab[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (ab[c] != AB_SPECIAL) band_counts_add<J>(ab[c] >> 16, ab[c] & 0xFFFFu, nn, (u64)(n - 1), acc[c]);
        }
    }
#pragma unroll
    for (int j = 0; j < J - 1; ++j) {
        const u64 v[4] = {acc[0][j], acc[1][j], acc[2][j], acc[3][j]};
        fold_store_w<64, 16, 4, 4, 65>(&red[0][0], x, y, v, (i64)blockIdx.x * 64, m, out + j, J - 1, first);
    }
}

// ---------------------------------------------------------------------------------------------------
// AB2 image: block = 64 targets x 16 row slices
// ---------------------------------------------------------------------------------------------------
template <int J>
__global__ __launch_bounds__(1024) void rank_accumulate2_kernel(AB2 ab, const u32 *__restrict__ nnan,
                                                                i64 rows, i64 n, const i64 *__restrict__ targets,
                                                                i64 tbegin, i64 m, u64 *__restrict__ out, int first) {
    __shared__ u64 red[16][64];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const i64 q = (i64)blockIdx.x * 64 + x;
    const i64 i = (q < m) ? (targets ? targets[q] : tbegin + q) : 0;
    u64 acc[JMAX - 1];
#pragma unroll
    for (int j = 0; j < JMAX - 1; ++j) acc[j] = 0;
    if (q < m)
        fold_rows<16, 8>(
            rows, y, [&](i64 r) { return FoldLoad<u32>{ab2_word(ab, r * n + i), nnan[r]}; },
            [&](const FoldLoad<u32> &v, i64 r) { fold_ab2<J>(v.w, v.nn, n, ab.A + r * n + i, acc); });
#pragma unroll
    for (int j = 0; j < J - 1; ++j) fold_store(red, x, y, acc[j], q < m, out + q * (J - 1) + j, first);
}

// The same fold for a contiguous, 4-aligned block of targets (the usual call: every curve): a thread takes FOUR neighbouring
// curves through 16-byte loads, so half a wave reads 512 bytes of a row instead of 128.  block = 32 quads x 16 row slices;
// needs n % 4 == 0 and tbegin % 4 == 0 (the image rows stay 16-byte aligned).  J <= 3 (accumulators in registers).
// One curve of the four at a time goes through the reduction: 4 KiB of LDS.
template <int J>
__global__ __launch_bounds__(512) void rank_accumulate2x4_kernel(AB2 ab, const u32 *__restrict__ nnan, i64 rows, i64 n,
                                                                  i64 tbegin, i64 m, u64 *__restrict__ out, int first) {
    __shared__ u64 red[16][32];
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
    const i64 q0 = ((i64)blockIdx.x * 32 + x) * 4;                    // first of this thread's four targets
    const i64 i0 = tbegin + q0;
    u64 acc[4][JMAX - 1];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < JMAX - 1; ++j) acc[c][j] = 0;
    if (q0 < m) {
        const uint4 *img = reinterpret_cast<const uint4 *>(ab.B);
        const uint2 *himg = reinterpret_cast<const uint2 *>(ab.H);
        fold_rows<16, 4>(
            rows, y,
            // four half words (8-byte loads) where there is a half-word image
            [&](i64 r) {
                const i64 at = r * n + i0;
                if (!himg) return FoldLoad<uint4>{img[at >> 2], nnan[r]};
                const uint2 h = himg[at >> 2];
                return FoldLoad<uint4>{make_uint4(ab2_word(h.x & 0xFFFFu, ab.B, at), ab2_word(h.x >> 16, ab.B, at + 1),
                                                  ab2_word(h.y & 0xFFFFu, ab.B, at + 2), ab2_word(h.y >> 16, ab.B, at + 3)),
                                       nnan[r]};
            },
            [&](const FoldLoad<uint4> &v, i64 r) {
                const u32 ww[4] = {v.w.x, v.w.y, v.w.z, v.w.w};
#pragma unroll
                for (int c = 0; c < 4; ++c) fold_ab2<J>(ww[c], v.nn, n, ab.A + r * n + i0 + c, acc[c]);
            });
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < J - 1; ++j) fold_store(red, x, y, acc[c][j], q0 + c < m, out + (q0 + c) * (J - 1) + j, first);
}

// The fold over the HALF-WORD image for a contiguous, 8-aligned block of targets: a thread takes EIGHT neighbouring curves
// through 16-byte loads (16 lanes read 256 bytes of a row); block = 16 octets x 32 row slices.  A marker among the eight (NaN
// / tied key: rare) sends that load through the B words.  Needs n % 8 == 0 and tbegin % 8 == 0.  J <= 3.
template <int J>
__global__ __launch_bounds__(512) void rank_accumulate_h8_kernel(AB2 ab, const u32 *__restrict__ nnan, i64 rows, i64 n,
                                                                 i64 tbegin, i64 m, u64 *__restrict__ out, int first) {
    __shared__ u64 red[32][16][9];                                    // (+1: the row slices fall on different banks)
    const int x = threadIdx.x & 15, y = threadIdx.x >> 4;
    const i64 q0 = ((i64)blockIdx.x * 16 + x) * 8;                    // first of this thread's eight targets
    const i64 i0 = tbegin + q0;
    u64 acc[8][JMAX - 1];
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int j = 0; j < JMAX - 1; ++j) acc[c][j] = 0;
    if (q0 < m) {
        const uint4 *himg = reinterpret_cast<const uint4 *>(ab.H);
        const u32 nm1 = (u32)n - 1u;
        auto fold8 = [&](const FoldLoad<uint4> &v, i64 row) {
            const u32 p[4] = {v.w.x, v.w.y, v.w.z, v.w.w}, nn = v.nn;
            u32 anym = 0;                                             // a half word 0xFFFF <=> a zero half word in ~p
#pragma unroll
            for (int k = 0; k < 4; ++k) anym |= ((~p[k]) - 0x00010001u) & p[k] & 0x80008000u;
            if (J == 2 && nn == 0 && !anym) {
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const u32 h = (c & 1) ? (p[c >> 1] >> 16) : (p[c >> 1] & 0xFFFFu);
                    acc[c][0] += (u64)h * (u64)(nm1 - h);              // untied keys of a NaN-free row: A * B
                }
                return;
            }
            // markers: the eight B words, and the eight A words when one of them is tied, through 16-byte loads as well (a
            // tie-heavy row is markers throughout)
            u32 bw[8] = {0, 0, 0, 0, 0, 0, 0, 0}, aw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (anym) {
                const uint4 *bp = reinterpret_cast<const uint4 *>(ab.B + row * n + i0);
                const uint4 b0 = bp[0], b1 = bp[1];
                bw[0] = b0.x; bw[1] = b0.y; bw[2] = b0.z; bw[3] = b0.w; bw[4] = b1.x; bw[5] = b1.y; bw[6] = b1.z; bw[7] = b1.w;
                bool anyt = false;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const u32 h = (c & 1) ? (p[c >> 1] >> 16) : (p[c >> 1] & 0xFFFFu);
                    anyt |= h == (u32)AB2_H_WORD && ab2_tied(bw[c]);
                }
                if (anyt) {
                    const uint4 *ap = reinterpret_cast<const uint4 *>(ab.A + row * n + i0);
                    const uint4 a0 = ap[0], a1 = ap[1];
                    aw[0] = a0.x; aw[1] = a0.y; aw[2] = a0.z; aw[3] = a0.w; aw[4] = a1.x; aw[5] = a1.y; aw[6] = a1.z; aw[7] = a1.w;
                }
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const u32 h = (c & 1) ? (p[c >> 1] >> 16) : (p[c >> 1] & 0xFFFFu);
                fold_ab2<J>(ab2_word(h, bw, c), nn, n, &aw[c], acc[c]);
            }
        };
        fold_rows<32, 4>(
            rows, y, [&](i64 r) { return FoldLoad<uint4>{himg[(r * n + i0) >> 3], nnan[r]}; }, fold8);
    }
#pragma unroll
    for (int j = 0; j < J - 1; ++j) {
        u64 v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = acc[c][j];
        fold_store_w<32, 16, 8, 9, 16 * 9>(&red[0][0][0], x, y, v, (i64)blockIdx.x * 128, m, out + j, J - 1, first);
    }
}

// ---------------------------------------------------------------------------------------------------
// host side: out (=|+=, first) the band counts of the targets over the rows of one pair image
// ---------------------------------------------------------------------------------------------------
int fold_pair_image(const u32 *AB, const u32 *nnan, i64 rows, i64 n, const i64 *targets, i64 tbegin, i64 m, int J, u64 *out,
                    int first, hipStream_t s) {
    dim3 grid((unsigned)((m + 63) / 64));
    if (!targets && (n % 4) == 0 && (tbegin % 4) == 0 && (m % 4) == 0 && J <= 3) {
        SD_DISPATCH_J(J, hipLaunchKernelGGL((rank_accumulate4_kernel<J_>), grid, dim3(1024), 0, s, AB, nnan, rows, n, tbegin, m,
                                            out, first));
    } else {
        SD_DISPATCH_J(J, hipLaunchKernelGGL((rank_accumulate_kernel<J_>), grid, dim3(1024), 0, s, AB, nnan, rows, n, targets,
                                            tbegin, m, out, first));
    }
    SD_HIP(hipGetLastError());
    return SD_OK;
}

int fold_ab2_image(const AB2 &ab, const u32 *nnan, i64 rows, i64 n, const i64 *targets, i64 tbegin, i64 m, int J, u64 *out,
                   int first, hipStream_t s) {
    if (ab.H && !targets && (n & 7) == 0 && (tbegin & 7) == 0 && J <= 3) {
        dim3 grid8((unsigned)((m + 127) / 128));
        if (J == 2) hipLaunchKernelGGL((rank_accumulate_h8_kernel<2>), grid8, dim3(512), 0, s, ab, nnan, rows, n, tbegin, m, out, first);
        else hipLaunchKernelGGL((rank_accumulate_h8_kernel<3>), grid8, dim3(512), 0, s, ab, nnan, rows, n, tbegin, m, out, first);
    } else if (!targets && (n & 3) == 0 && (tbegin & 3) == 0 && J <= 3) {
        dim3 grid4((unsigned)((m + 127) / 128));
        if (J == 2) hipLaunchKernelGGL((rank_accumulate2x4_kernel<2>), grid4, dim3(512), 0, s, ab, nnan, rows, n, tbegin, m, out, first);
        else hipLaunchKernelGGL((rank_accumulate2x4_kernel<3>), grid4, dim3(512), 0, s, ab, nnan, rows, n, tbegin, m, out, first);
    } else {
        dim3 grid((unsigned)((m + 63) / 64));
        SD_DISPATCH_J(J, hipLaunchKernelGGL((rank_accumulate2_kernel<J_>), grid, dim3(1024), 0, s, ab, nnan, rows, n, targets,
                                            tbegin, m, out, first));
    }
    SD_HIP(hipGetLastError());
    return SD_OK;
}

}  // namespace sd
