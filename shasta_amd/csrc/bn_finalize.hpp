// One channel of a batch-statistics BatchNorm's finalize, shared by bn_rows.hip (BatchNorm1d over feature rows), bn_maps.hip
// (BatchNorm2d over NCHW maps) and bn_sync.hip (either, merged over ranks): mean / M2 / n of the whole batch -> what the normalisation
// uses (mean, 1 / sqrt(biased variance + eps)) and the running statistics as torch keeps them ((1 - m) r + m new, unbiased variance); the
// blend is evaluated in float64 and rounded once.  NULL running pointers skip the update.
#pragma once
#include "common.hpp"

namespace shasta {

// (mean, m2) in registers: bn_sync.hip merges them over the ranks' records first
__device__ __forceinline__ void bn_finalize_channel(float mean, float m2, int C, int c, double n, float eps, float momentum,
                                                    float* __restrict__ stat, float* __restrict__ running_mean,
                                                    float* __restrict__ running_var) {
    const float var = (float)((double)m2 / n);
    stat[c] = mean;
    stat[C + c] = 1.0f / sqrtf(var + eps);
    const double m = (double)momentum;
    if (running_mean) running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * (double)mean);
    if (running_var) running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * ((double)m2 / (n > 1.0 ? n - 1.0 : 1.0)));
}

__device__ __forceinline__ void bn_finalize_channel(const float* __restrict__ mean_m2, int C, int c, double n, float eps, float momentum,
                                                    float* __restrict__ stat, float* __restrict__ running_mean,
                                                    float* __restrict__ running_var) {
    bn_finalize_channel(mean_m2[c], mean_m2[C + c], C, c, n, eps, momentum, stat, running_mean, running_var);
}

}  // namespace shasta
