// Synchronised batch statistics: the finalize of a batch-statistics BatchNorm whose batch is spread over R ranks (the reference converts
// every BatchNorm of the model with apex.parallel.convert_syncbn_model before DDP, tools/nusc_shasta/train.py:155-156, so the frozen
// backbone's BatchNorm1d and the frozen neck's BatchNorm2d normalise with the statistics of the GLOBAL batch).  It takes the place of
// step 3 of bn_rows.hip / bn_maps.hip: each rank runs its stats kernel into the front of its RECORD, the records are all-gathered, and
// every rank runs this kernel on the same gathered bytes - so stat and the running statistics are bit-equal across ranks by construction.
//
// RECORD of one rank, 8 C + 8 bytes, 8-byte aligned: float mean[C], float M2[C] (what the stats kernels write to mean_m2), then the
// rank's value count as one int64 (an int64, not a float: counts beyond 2^24 must merge exactly).  R records in rank order.
//
// One thread per channel, float64.  The records are merged SEQUENTIALLY in rank order with Chan's update, records of count 0 skipped:
// the first non-empty record is taken as it is, so for R = 1 (and for any number of empty ranks around one full one) the merge is the
// identity and the result has the bits of the plain finalize on the same mean_m2 and n; n mean / n would not be.  Merged mean and M2 are
// rounded once to fp32, the rest is bn_finalize_channel with n = N.  A total count of 0 or a negative count (the modules never produce
// either) writes NaN to stat and leaves the running statistics and the counter alone: loud downstream, no fault, no host read.
#include "bn_finalize.hpp"

namespace shasta {

constexpr int BNS_THREADS = 128;
constexpr int BNS_MAX_RANKS = 64;

static bool bns_channels_ok(int C) { return C >= 16 && C <= 1024 && C % 16 == 0; }

__global__ __launch_bounds__(BNS_THREADS) void bn_sync_finalize_kernel(const char* __restrict__ records, int R, int C, float eps, float momentum,
                                                                       float* __restrict__ stat, float* __restrict__ mean_m2,
                                                                       long* __restrict__ n_total, float* __restrict__ running_mean,
                                                                       float* __restrict__ running_var, long* __restrict__ nbt) {
    const int c = blockIdx.x * BNS_THREADS + threadIdx.x;
    if (c >= C) return;
    const size_t stride = (size_t)8 * C + 8;
    long total = 0;
    bool bad = false;
    for (int r = 0; r < R; ++r) {
        const long n_r = *reinterpret_cast<const long*>(records + r * stride + (size_t)8 * C);
        bad |= n_r < 0;
        total += n_r;
    }
    bad |= total <= 0;
    if (c == 0 && n_total) n_total[0] = bad ? 0 : total;
    if (bad) {
        const float nan = __builtin_nanf("");
        stat[c] = nan;
        stat[C + c] = nan;
        if (mean_m2) {
            mean_m2[c] = nan;
            mean_m2[C + c] = nan;
        }
        return;
    }
    double N = 0.0, mean = 0.0, m2 = 0.0;
    for (int r = 0; r < R; ++r) {
        const float* rec = reinterpret_cast<const float*>(records + r * stride);
        const long cnt = *reinterpret_cast<const long*>(records + r * stride + (size_t)8 * C);
        if (cnt == 0) continue;
        const double n_r = (double)cnt, mean_r = (double)rec[c], m2_r = (double)rec[C + c];
        if (N == 0.0) {  // the first non-empty record, as it is
            N = n_r;
            mean = mean_r;
            m2 = m2_r;
            continue;
        }
        const double d = mean_r - mean, Nn = N + n_r;
        mean += d * n_r / Nn;
        m2 += m2_r + d * d * N * n_r / Nn;
        N = Nn;
    }
    const float mean_f = (float)mean, m2_f = (float)m2;
    if (mean_m2) {
        mean_m2[c] = mean_f;
        mean_m2[C + c] = m2_f;
    }
    bn_finalize_channel(mean_f, m2_f, C, c, N, eps, momentum, stat, running_mean, running_var);
    if (nbt && c == 0) nbt[0] += 1;
}

}  // namespace shasta

using namespace shasta;

extern "C" size_t shasta_bn_sync_record_bytes(int C) { return bns_channels_ok(C) ? (size_t)8 * C + 8 : 0; }

extern "C" int shasta_bn_sync_finalize_f32(const void* records, int R, int C, float eps, float momentum, float* stat, float* mean_m2,
                                           long* n_total, float* running_mean, float* running_var, long* num_batches_tracked,
                                           shasta_stream_t stream) {
    if (!bns_channels_ok(C) || R < 1 || R > BNS_MAX_RANKS) {
        set_error_msg("bn_sync_finalize: channel counts that are multiples of 16 from 16 to 1024, 1 to 64 records only");
        return SHASTA_E_UNSUPPORTED;
    }
    SHASTA_REQUIRE(records && stat, "bn_sync_finalize: null pointer");
    if ((uintptr_t)records % 8 || (uintptr_t)n_total % 8 || (uintptr_t)num_batches_tracked % 8) {
        set_error_msg("bn_sync_finalize: records, n_total and num_batches_tracked must be 8-byte aligned");
        return SHASTA_E_ALIGN;
    }
    hipLaunchKernelGGL(bn_sync_finalize_kernel, dim3(cdiv(C, BNS_THREADS)), dim3(BNS_THREADS), 0, as_stream(stream),
                       static_cast<const char*>(records), R, C, eps, momentum, stat, mean_m2, n_total, running_mean, running_var,
                       num_batches_tracked);
    return check_launch("bn_sync_finalize");
}
