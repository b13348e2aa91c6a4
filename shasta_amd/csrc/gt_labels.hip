// Ground-truth affinity labels on the device: what preprocessing/make_gt_shasta.py:81-152 computes per frame pair from
// preprocessing/gt_association/associate.py:6-80 (`distance_type="l2"`), for all frames of all scenes of a split in one call.
//
//   gt_associate_kernel  one wavefront per frame: detections in descending (score, index) order each take the nearest free
//                        ground-truth box of a compatible type, if it is nearer than the threshold      -> gt_of_det
//   gt_link_kernel       one workgroup per emitted frame: ground-truth ids of frames t-1 and t           -> col_of_prev, newborn
//
// float64 in numpy's operation order (dist = sqrt(dx*dx + dy*dy), products and sum rounded one by one: the build has
// -ffp-contract=off; the double sqrt is correctly rounded like numpy's), strict `<` in both tests, lowest ground-truth index among
// equal distances: the labels equal the reference's index for index.
#include <limits.h>

#include "common.hpp"

namespace shasta {

constexpr int GT_CAP_DET = 1024;  // detections per frame
constexpr int GT_CAP_GT = 512;    // ground-truth boxes per frame
constexpr int GT_LINK_THREADS = 256;

struct GtArgs {
    const double* det_xy;                // (total_det, 2)
    const double* det_score;             // (total_det,)
    const int* det_type;                 // (total_det,) index into type_mask
    const int* det_off;                  // (frames + 1,)
    const double* gt_xy;                 // (total_gt, 2)
    const int* gt_type;                  // (total_gt,) 0 .. 63
    const int* gt_id;                    // (total_gt,)
    const int* gt_off;                   // (frames + 1,)
    const unsigned long long* type_mask; // (n_det_types,) bit t: a detection of this type may take a ground-truth box of type t
    const int* has_prev;                 // (frames,)
    const int* emit;                     // (frames,)
    int* gt_of_det;                      // (total_det,)
    int* col_of_prev;                    // (total_det,)
    int* newborn;                        // (total_det,)
    double threshold;
    int n_det_types, frames, total_det, total_gt, max_det, max_gt;
};

// Static LDS of the association kernel, 46 080 bytes: three waves per CU.
struct GtAssocLds {
    double dx[GT_CAP_DET], dy[GT_CAP_DET], score[GT_CAP_DET];  // 24 576
    unsigned long long mask[GT_CAP_DET];                       //  8 192: the detection's row of the type table
    double gx[GT_CAP_GT], gy[GT_CAP_GT];                       //  8 192
    int order[GT_CAP_DET];                                     //  4 096: order[r] = the detection visited r-th
    unsigned char gtype[GT_CAP_GT], taken[GT_CAP_GT];          //  1 024
};

struct GtFrame {
    int d0, K, g0, G;
};

// The rows of frame f, or false when its offsets do not describe rows inside the arrays and the call's capacity: such a frame is
// skipped, nothing of it is read or written.
__device__ __forceinline__ bool gt_frame(const GtArgs& a, int f, GtFrame& fr) {
    const int d0 = a.det_off[f], d1 = a.det_off[f + 1], g0 = a.gt_off[f], g1 = a.gt_off[f + 1];
    fr = GtFrame{d0, d1 - d0, g0, g1 - g0};
    return d0 >= 0 && d1 >= d0 && d1 <= a.total_det && d1 - d0 <= a.max_det && g0 >= 0 && g1 >= g0 && g1 <= a.total_gt && g1 - g0 <= a.max_gt;
}

__global__ __launch_bounds__(64) void gt_associate_kernel(GtArgs a) {
    __shared__ GtAssocLds s;
    const int lane = threadIdx.x;
    GtFrame fr;
    if (!gt_frame(a, blockIdx.x, fr)) return;
    const int K = fr.K, G = fr.G;
    int* out = a.gt_of_det + fr.d0;
    for (int k = lane; k < K; k += 64) {
        s.dx[k] = a.det_xy[2 * (size_t)(fr.d0 + k)];
        s.dy[k] = a.det_xy[2 * (size_t)(fr.d0 + k) + 1];
        s.score[k] = a.det_score[fr.d0 + k];
        const int t = a.det_type[fr.d0 + k];
        s.mask[k] = t >= 0 && t < a.n_det_types ? a.type_mask[t] : 0ull;
        s.order[k] = -1;
        out[k] = -1;
    }
    for (int g = lane; g < G; g += 64) {
        s.gx[g] = a.gt_xy[2 * (size_t)(fr.g0 + g)];
        s.gy[g] = a.gt_xy[2 * (size_t)(fr.g0 + g) + 1];
        const int t = a.gt_type[fr.g0 + g];
        s.gtype[g] = t >= 0 && t < 64 ? (unsigned char)t : 255;  // 255: compatible with nothing
        s.taken[g] = 0;
    }
    __syncthreads();
    if (K == 0 || G == 0) return;  // everything on the other side is a false positive / false negative
    // rank sort: sorted((score, index))[::-1] - the higher score first, of equal scores the larger index first.  (A NaN score
    // compares false both ways and ranks collide: the slots left at -1 are skipped below and those detections stay unmatched.)
    for (int k = lane; k < K; k += 64) {
        const double sk = s.score[k];
        int r = 0;
        for (int j = 0; j < K; ++j) {
            const double sj = s.score[j];
            r += (sj > sk || (sj == sk && j > k)) ? 1 : 0;
        }
        s.order[r] = k;
    }
    __syncthreads();
    for (int r = 0; r < K; ++r) {
        const int k = s.order[r];
        if (k < 0) continue;
        const double px = s.dx[k], py = s.dy[k];
        const unsigned long long m = s.mask[k];
        double best = INFINITY;
        int bg = INT_MAX;
        for (int g = lane; g < G; g += 64) {
            const unsigned t = s.gtype[g];
            if (s.taken[g] || t >= 64 || !((m >> t) & 1ull)) continue;
            const double ex = s.gx[g] - px, ey = s.gy[g] - py;
            const double d = sqrt(ex * ex + ey * ey);
            if (d < best) {  // strict: of equal distances the lower index stays
                best = d;
                bg = g;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double od = __shfl_xor(best, off, 64);
            const int og = __shfl_xor(bg, off, 64);
            if (od < best || (od == best && og < bg)) {
                best = od;
                bg = og;
            }
        }
        if (best < a.threshold && lane == 0) {  // (best < threshold implies that some lane found a box: bg is an index)
            s.taken[bg] = 1;
            out[k] = bg;
        }
        __syncthreads();
    }
}

// From gt_of_det of frames t-1 and t and the ids of their ground-truth boxes (unique within a frame): the column of every previous
// detection - the current detection that took the box with the same id, K + 1 (false negative) when that id is in the current frame
// but no detection took it, K (dead) otherwise - and newborn = a matched current detection whose id no previous detection held.
__global__ __launch_bounds__(GT_LINK_THREADS) void gt_link_kernel(GtArgs a) {
    __shared__ int cur_id[GT_CAP_GT], cur_det[GT_CAP_GT], prev_id[GT_CAP_GT], prev_det[GT_CAP_GT];  // 8 192 bytes
    const int f = blockIdx.x, tid = threadIdx.x;
    if (!a.emit[f]) return;
    GtFrame c, p{0, 0, 0, 0};
    if (!gt_frame(a, f, c)) return;
    const bool has_prev = f > 0 && a.has_prev[f] != 0;
    if (has_prev && !gt_frame(a, f - 1, p)) return;
    for (int g = tid; g < c.G; g += GT_LINK_THREADS) {
        cur_id[g] = a.gt_id[c.g0 + g];
        cur_det[g] = -1;
    }
    for (int g = tid; g < p.G; g += GT_LINK_THREADS) {
        prev_id[g] = a.gt_id[p.g0 + g];
        prev_det[g] = -1;
    }
    __syncthreads();
    for (int k = tid; k < c.K; k += GT_LINK_THREADS) {
        const int g = a.gt_of_det[c.d0 + k];
        if (g >= 0 && g < c.G) cur_det[g] = k;
    }
    for (int n = tid; n < p.K; n += GT_LINK_THREADS) {
        const int g = a.gt_of_det[p.d0 + n];
        if (g >= 0 && g < p.G) prev_det[g] = n;
    }
    __syncthreads();
    for (int k = tid; k < c.K; k += GT_LINK_THREADS) {
        const int g = a.gt_of_det[c.d0 + k];
        int nb = 0;
        if (g >= 0 && g < c.G) {
            nb = 1;
            const int id = cur_id[g];
            for (int q = 0; q < p.G; ++q)
                if (prev_id[q] == id && prev_det[q] >= 0) nb = 0;
        }
        a.newborn[c.d0 + k] = nb;
    }
    if (!has_prev) return;
    for (int n = tid; n < p.K; n += GT_LINK_THREADS) {
        const int gp = a.gt_of_det[p.d0 + n];
        int col = c.K;
        if (gp >= 0 && gp < p.G) {
            const int id = prev_id[gp];
            for (int g = 0; g < c.G; ++g)
                if (cur_id[g] == id) {
                    col = cur_det[g] >= 0 ? cur_det[g] : c.K + 1;
                    break;
                }
        }
        a.col_of_prev[p.d0 + n] = col;
    }
}

}  // namespace shasta

using namespace shasta;

extern "C" int shasta_gt_labels_f64(const double* det_xy, const double* det_score, const int32_t* det_type, const int32_t* det_off,
                                    const double* gt_xy, const int32_t* gt_type, const int32_t* gt_id, const int32_t* gt_off,
                                    const uint64_t* type_mask, int n_det_types, const int32_t* has_prev, const int32_t* emit, int frames,
                                    int total_det, int total_gt, int max_det, int max_gt, double threshold, int32_t* gt_of_det,
                                    int32_t* col_of_prev, int32_t* newborn, shasta_stream_t stream) {
    SHASTA_REQUIRE(frames >= 0 && total_det >= 0 && total_gt >= 0 && max_det >= 0 && max_gt >= 0 && n_det_types >= 0, "gt_labels: bad size");
    SHASTA_REQUIRE(threshold == threshold, "gt_labels: NaN threshold");
    if (max_det > GT_CAP_DET || max_gt > GT_CAP_GT) {
        set_error_msg("gt_labels: at most 1024 detections and 512 ground-truth boxes per frame (a frame's association state lives in LDS)");
        return SHASTA_E_UNSUPPORTED;
    }
    if (frames == 0) return SHASTA_OK;
    SHASTA_REQUIRE(det_off && gt_off && has_prev && emit, "gt_labels: null pointer");
    SHASTA_REQUIRE(total_det == 0 || (det_xy && det_score && det_type && gt_of_det && col_of_prev && newborn), "gt_labels: null pointer");
    SHASTA_REQUIRE(total_gt == 0 || (gt_xy && gt_type && gt_id), "gt_labels: null pointer");
    SHASTA_REQUIRE(n_det_types == 0 || type_mask, "gt_labels: null pointer");
    if (reinterpret_cast<uintptr_t>(type_mask) % 8 != 0) {
        set_error_msg("gt_labels: type_mask must be 8-byte aligned");
        return SHASTA_E_ALIGN;
    }
    GtArgs a{det_xy, det_score, det_type, det_off, gt_xy, gt_type, gt_id, gt_off, reinterpret_cast<const unsigned long long*>(type_mask),
             has_prev, emit, gt_of_det, col_of_prev, newborn, threshold, n_det_types, frames, total_det, total_gt, max_det, max_gt};
    hipLaunchKernelGGL(gt_associate_kernel, dim3(frames), dim3(64), 0, as_stream(stream), a);
    const int rc = check_launch("gt_associate");
    if (rc != SHASTA_OK) return rc;
    hipLaunchKernelGGL(gt_link_kernel, dim3(frames), dim3(GT_LINK_THREADS), 0, as_stream(stream), a);
    return check_launch("gt_link");
}
