// prob_common.h -- device helpers shared by the probabilistic depths (prob_depth.hip: K8, prob_band.hip: K9).
#pragma once
#include "sd_common.h"

namespace sd {

// Phi(x), the standard normal CDF, from erfc: accurate to a few ulp in the lower tail; Phi(-x) gives the upper tail
// with the same accuracy (never 1 - Phi(x))
__device__ __forceinline__ double pr_phi(double x) { return 0.5 * erfc(-x * M_SQRT1_2); }

// block-wide sum of v over 256 threads in a fixed order; every lane gets the result
__device__ __forceinline__ double pr_block_sum(double v, double *scratch) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int k = 0; k < 4; ++k) r += scratch[k];                    // every lane, same order (256 threads = 4 waves)
    __syncthreads();
    return r;
}

}  // namespace sd
