// projection_select.h -- K12's median and MAD by selection from a sorted sequence, and the outlyingness (internal).
//
// Shared by K12 (projection.hip: sorted global rows, rows with one value inserted, sorted LDS blocks) and K18
// (multi_cloud.hip: a cloud's projections sorted in LDS).  The definition and its roundings are stated at the top of
// projection.hip; device code but for one launcher.  K23 (curve_project.hip) takes pd_outlyingness and that launcher for the
// projections of curves.
#pragma once
#include "sd_common.h"

namespace sd {
// pd_locscale_kernel (projection.hip): med[r], mad[r] of the kk rows of K (kk x n), every row sorted ascending
int launch_pd_locscale(const double *K, i64 n, int kk, double *med, double *mad, hipStream_t s);
}  // namespace sd

#ifdef __HIPCC__
namespace sd {

struct PdGlobalRow {                                               // a sorted row in global memory
    const double *p;
    __device__ __forceinline__ double operator()(i64 i) const { return p[i]; }
};

struct PdInsertedRow {                                             // ... with v virtually inserted at position pos
    const double *p;
    i64 pos;
    double v;
    __device__ __forceinline__ double operator()(i64 i) const { return i < pos ? p[i] : i == pos ? v : p[i - 1]; }
};

struct PdLdsRow {                                                  // a sorted array in LDS
    const double *p;
    __device__ __forceinline__ double operator()(i64 i) const { return p[(int)i]; }
};

// Partition point of a predicate that holds on a prefix of [lo, hi) and fails behind it: the first index where it
// fails (hi when there is none).  Two searchers with the same result:
struct PdSerialSearch {                                            // one thread, a binary search
    template <class Pred>
    __device__ __forceinline__ i64 operator()(i64 lo, i64 hi, Pred pred) const {
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if (pred(mid)) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    }
};

// one full wave64 with wave-uniform lo and hi: per round the 64 lanes probe 64 evenly spaced positions, so a range of
// 2^24 is settled in 4 rounds of one dependent read each instead of 24; every lane returns the result
struct PdWaveSearch {
    template <class Pred>
    __device__ __forceinline__ i64 operator()(i64 lo, i64 hi, Pred pred) const {
        const int lane = threadIdx.x & 63;
        while (lo < hi) {
            const i64 step = (hi - lo + 63) >> 6;
            const i64 p = lo + (lane + 1) * step - 1;               // lane's probe; the probes below hi are a prefix of the lanes
            const bool t = p < hi && pred(p);
            const int c = __popcll(__ballot(t));                    // the predicate's prefix: lanes 0 .. c - 1
            lo += c * step;                                         // probe c - 1 held: the partition point is behind it
            const i64 pc = lo + step - 1;                           // probe c failed (or lies at or behind hi)
            hi = pc < hi ? pc : hi;
        }
        return lo;
    }
};

// first index of [0, N) whose value is not below key (N when there is none)
template <class S, class Search = PdSerialSearch>
__device__ __forceinline__ i64 pd_lower_bound(const S s, i64 N, double key, Search search = Search()) {
    return search(0, N, [&](i64 i) { return s(i) < key; });
}

// med and mad of the sorted sequence s(0) <= ... <= s(N - 1), N >= 1
template <class S, class Search = PdSerialSearch>
__device__ __forceinline__ void pd_locscale(const S s, i64 N, double &med, double &mad, Search search = Search()) {
    const i64 k1 = (N - 1) >> 1, k2 = N >> 1;
    med = k1 == k2 ? s(k1) : __dmul_rn(__dadd_rn(s(k1), s(k2)), 0.5);
    const double m = med;
    const i64 a = pd_lower_bound(s, N, m, search);
    const i64 la = a, lb = N - a;
    // A(j) = med - s(a - 1 - j), j < la;  B(j) = s(a + j) - med, j < lb;  both ascending
    // i = how many of the k1 smallest deviations come from A (ties: A first): the merge-path split
    const i64 lo = search(k1 > lb ? k1 - lb : 0, k1 < la ? k1 : la, [&](i64 mid) {
        return __dsub_rn(m, s(a - 1 - mid)) <= __dsub_rn(s(a + (k1 - 1 - mid)), m);
    });
    i64 i = lo, j = k1 - lo;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    double av = i < la ? __dsub_rn(med, s(a - 1 - i)) : inf;
    double bv = j < lb ? __dsub_rn(s(a + j), med) : inf;
    const double e1 = av <= bv ? av : bv;                           // the k1-th smallest deviation (from 0)
    if (k1 == k2) {
        mad = e1;
        return;
    }
    if (av <= bv) {
        ++i;
        av = i < la ? __dsub_rn(med, s(a - 1 - i)) : inf;
    } else {
        ++j;
        bv = j < lb ? __dsub_rn(s(a + j), med) : inf;
    }
    const double e2 = av <= bv ? av : bv;
    mad = __dmul_rn(__dadd_rn(e1, e2), 0.5);
}

__device__ __forceinline__ double pd_outlyingness(double z, double med, double mad) {
    const double num = fabs(__dsub_rn(z, med));
    if (num == 0.0) return 0.0;
    if (mad == 0.0) return __longlong_as_double(0x7ff0000000000000LL);
    return __ddiv_rn(num, mad);
}

}  // namespace sd
#endif
