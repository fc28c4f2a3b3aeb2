// multi_cloud_batches.h -- the one batch loop of K18 (multi_cloud.hip) and the seam its consumers plug into (internal).
// Included by multi_cloud.hip and directional_out.hip alone: the consumer is a std::function, and sd_common.h, which every
// device translation unit includes, stays free of the C++ standard library.
#pragma once
#include <functional>
#include "sd_common.h"

namespace sd {

// The one batch loop of K18 and what it hands to its consumer once per batch, in stream order, after the last slice of
// the batch has been launched: the values of EVERY curve at the batch's timepoints t0 .. t0 + tb - 1 and the batch's points.
struct McBatch {
    const void *V;                                                 // V[tb][i]: u32 (lds) or int64 (global) counts, or the outlyingness
    const double *pts;                                             // lds: Y[tb][e][i], feature-major;  global: C[i][e], tb = 1
    bool feature_major;
    void *extra;                                                   // the consumer's own bytes (nullptr when it asked for none)
    i64 t0, tb;
};
typedef std::function<int(const McBatch &, hipStream_t)> McConsumer;
int launch_multi_cloud_batches(bool proj, int route, const double *P, i64 n, i64 T, int d, const double *U, i64 k, size_t extra,
                               const McConsumer &consume, void *ws, size_t ws_bytes, hipStream_t s);

}  // namespace sd
