// CenterPoint head losses (FastFocalLoss + RegLoss) with the gradient with respect to the head's raw outputs, all tasks of a batch in
// one chain (include/shasta_hip.h has the formulas).  Chain, no host read:
//   1. cl_count_kernel  : one workgroup per task: num_pos = number of slots with mask != 0 (integers).
//   2. cl_dense_kernel  : CL_BLOCKS workgroups per task, grid-stride over the task's B C H W logits: every logit and target is read once,
//        sigma = 1 / (1 + expf(-x)), p = clamp(sigma), L = log1pf(-p); the term L p^2 (1 - t)^4 goes into a float64 accumulator, and
//        d loss / d x = -(1 - t)^4 (2 p^2 (1 - p) L - p^3) / num_pos is stored (0 where sigma lies outside the clamp's closed interval).
//   3. cl_sparse_kernel : one workgroup per (sample, task): one thread per slot gathers the logit and the ten box channels at its
//        pixel; the first slot of every pixel (and class) adds the terms of all slots that share it IN SLOT ORDER and stores once -
//        no atomics.  Eleven float64 sums (pos, |pred - target| per channel) per workgroup.
//   4. cl_final_kernel  : one workgroup per task combines the partials in a fixed tree and writes the task's 14 results.
#include "common.hpp"
#include <math.h>

namespace shasta {

constexpr int CL_THREADS = 256;
constexpr int CL_BLOCKS = 128;  // dense workgroups per task: fixed, so the summation tree depends on nothing but the shape
constexpr int CL_SUMS = 11;     // pos, then the ten box channels
static_assert(sizeof(shasta_center_loss_task) == 160, "table layout");

struct ClTable {
    shasta_center_loss_task t[SHASTA_CENTER_MAX_TASKS];
};

struct ClCodeWeights {
    float w[10];
};

struct ClWs {
    int32_t* num_pos;  // T
    double* neg;       // T * CL_BLOCKS
    double* sums;      // T * B * CL_SUMS
    size_t bytes;
    ClWs(void* base, int T, int B) {
        char* p = static_cast<char*>(base);
        size_t at = 0;
        auto take = [&](size_t n) { char* q = p + at; at += align_up(n, 256); return q; };
        num_pos = reinterpret_cast<int32_t*>(take(SHASTA_CENTER_MAX_TASKS * sizeof(int32_t)));
        neg = reinterpret_cast<double*>(take((size_t)T * CL_BLOCKS * sizeof(double)));
        sums = reinterpret_cast<double*>(take((size_t)T * B * CL_SUMS * sizeof(double)));
        bytes = at;
    }
};

static bool cl_sizes_ok(int T, int B) { return T >= 1 && T <= SHASTA_CENTER_MAX_TASKS && B >= 1 && B <= SHASTA_CENTER_MAX_BATCH; }

// sum over the 256 threads in a fixed tree (butterfly inside a wave, then (w0 + w1) + (w2 + w3)); result in every thread
__device__ __forceinline__ double cl_block_sum(double v, double* s_w) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();  // (s_w may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

constexpr float CL_PMIN = 1e-4f, CL_PMAX = (float)(1.0 - 1e-4);

// p = clamp(sigmoid(x)); *pass = 1 where the clamp passes the gradient (its closed interval), else 0
__device__ __forceinline__ float cl_prob(float x, float* pass) {
    const float s = 1.0f / (1.0f + expf(-x));
    *pass = (s >= CL_PMIN && s <= CL_PMAX) ? 1.0f : 0.0f;
    return fminf(fmaxf(s, CL_PMIN), CL_PMAX);
}

__device__ __forceinline__ float cl_grad_scale(int num_pos) { return num_pos > 0 ? -1.0f / (float)num_pos : -1.0f; }

static __global__ __launch_bounds__(CL_THREADS) void cl_count_kernel(ClTable tab, int slots, int32_t* __restrict__ num_pos) {
    __shared__ double s_w[4];
    const uint8_t* mask = tab.t[blockIdx.x].mask;
    int c = 0;
    for (int i = threadIdx.x; i < slots; i += CL_THREADS) c += mask[i] != 0;
    const double total = cl_block_sum((double)c, s_w);  // integers below 2^53: exact
    if (threadIdx.x == 0) num_pos[blockIdx.x] = (int)total;
}

static __global__ __launch_bounds__(CL_THREADS) void cl_dense_kernel(ClTable tab, int B, int HW, const int32_t* __restrict__ num_pos,
                                                                     double* __restrict__ neg) {
    __shared__ double s_w[4];
    const shasta_center_loss_task& K = tab.t[blockIdx.y];
    const long long per = (long long)K.num_class * HW, total = per * B;
    const float scale = cl_grad_scale(num_pos[blockIdx.y]);
    double acc = 0.0;
    for (long long e = (long long)blockIdx.x * CL_THREADS + threadIdx.x; e < total; e += (long long)CL_BLOCKS * CL_THREADS) {
        const long long b = e / per, rem = e - b * per;
        const float x = K.hm[b * K.hm_stride + rem], t = K.target_hm[e];
        float pass;
        const float p = cl_prob(x, &pass);
        const float L = log1pf(-p);
        const float u = 1.0f - t, u2 = u * u, u4 = u2 * u2, p2 = p * p;
        acc += (double)(L * p2 * u4);
        const float g = u4 * (2.0f * p2 * (1.0f - p) * L - p2 * p);
        K.g_hm[e] = pass * (scale * g);
    }
    const double sum = cl_block_sum(acc, s_w);
    if (threadIdx.x == 0) neg[(size_t)blockIdx.y * CL_BLOCKS + blockIdx.x] = sum;
}

static __global__ __launch_bounds__(CL_THREADS) void cl_sparse_kernel(ClTable tab, int B, int H, int W, int max_objs, float weight,
                                                                      ClCodeWeights cw, const int32_t* __restrict__ num_pos,
                                                                      double* __restrict__ sums) {
    __shared__ double s_w[4];
    __shared__ int s_ind[SHASTA_CENTER_MAX_OBJS];   // the slot's pixel, -1: nothing to add
    __shared__ int s_cat[SHASTA_CENTER_MAX_OBJS];
    __shared__ float s_gpos[SHASTA_CENTER_MAX_OBJS];
    __shared__ uint32_t s_sgn[SHASTA_CENTER_MAX_OBJS];  // two bits per box channel: 1 = +, 2 = -, 0 = no gradient
    const int b = blockIdx.x, task = blockIdx.y, HW = H * W;
    const shasta_center_loss_task& K = tab.t[task];
    const int np = num_pos[task];
    const float scale = cl_grad_scale(np);
    const float box_scale = weight / ((float)np + 1e-4f);
    const int head_of[10] = {0, 0, 1, 2, 2, 2, 3, 3, 4, 4}, chan_of[10] = {0, 1, 0, 0, 1, 2, 0, 1, 0, 1};
    double part[CL_SUMS];
#pragma unroll
    for (int c = 0; c < CL_SUMS; ++c) part[c] = 0.0;
    for (int k = threadIdx.x; k < max_objs; k += CL_THREADS) {
        const size_t slot = (size_t)b * max_objs + k;
        const long long ind = K.ind[slot], cat = K.cat[slot];
        const bool valid = K.mask[slot] != 0 && ind >= 0 && ind < HW && cat >= 0 && cat < K.num_class;
        s_ind[k] = valid ? (int)ind : -1;
        s_cat[k] = valid ? (int)cat : -1;
        float gpos = 0.0f;
        uint32_t sgn = 0;
        if (valid) {
            float pass;
            const float q = cl_prob(K.hm[(long long)b * K.hm_stride + cat * HW + ind], &pass);
            const float lq = logf(q), r = 1.0f - q, r2 = r * r;
            part[0] += (double)(lq * r2);
            gpos = pass * (scale * (r2 * r - 2.0f * q * r2 * lq));
#pragma unroll
            for (int c = 0; c < 10; ++c) {
                const float pred = K.box[head_of[c]][(long long)b * K.box_stride[head_of[c]] + (long long)chan_of[c] * HW + ind];
                const float d = pred - K.anno_box[slot * 10 + c];
                part[1 + c] += (double)fabsf(d);
                sgn |= (d > 0.0f ? 1u : d < 0.0f ? 2u : 0u) << (2 * c);
            }
        }
        s_gpos[k] = gpos;
        s_sgn[k] = sgn;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < max_objs; k += CL_THREADS) {
        const int ind = s_ind[k], cat = s_cat[k];
        if (ind < 0) continue;
        bool first_px = true, first_hm = true;
        for (int j = 0; j < k; ++j)
            if (s_ind[j] == ind) {
                first_px = false;
                if (s_cat[j] == cat) first_hm = false;
            }
        if (!first_hm) continue;  // (a slot that is not the first of its pixel and class is not the first of its pixel either)
        float* gh = K.g_hm + ((size_t)b * K.num_class + cat) * HW + ind;
        float acc_h = *gh;  // the dense pass's value
        float acc_b[10];
#pragma unroll
        for (int c = 0; c < 10; ++c) acc_b[c] = 0.0f;
        for (int j = k; j < max_objs; ++j) {
            if (s_ind[j] != ind) continue;
            if (s_cat[j] == cat) acc_h += s_gpos[j];
            if (first_px) {
                const uint32_t sg = s_sgn[j];
#pragma unroll
                for (int c = 0; c < 10; ++c) {
                    const uint32_t two = (sg >> (2 * c)) & 3u;
                    const float step = box_scale * cw.w[c];
                    acc_b[c] += two == 1u ? step : two == 2u ? -step : 0.0f;
                }
            }
        }
        *gh = acc_h;
        if (first_px) {
#pragma unroll
            for (int c = 0; c < 10; ++c) K.g_box[((size_t)b * 10 + c) * HW + ind] = acc_b[c];
        }
    }
#pragma unroll
    for (int c = 0; c < CL_SUMS; ++c) {
        const double s = cl_block_sum(part[c], s_w);
        if (threadIdx.x == 0) sums[((size_t)task * B + b) * CL_SUMS + c] = s;
    }
}

static __global__ __launch_bounds__(CL_THREADS) void cl_final_kernel(int B, float weight, ClCodeWeights cw, const int32_t* __restrict__ num_pos,
                                                                     const double* __restrict__ neg, const double* __restrict__ sums,
                                                                     float* __restrict__ out) {
    __shared__ double s_w[4];
    const int task = blockIdx.x;
    const double n = cl_block_sum(threadIdx.x < CL_BLOCKS ? neg[(size_t)task * CL_BLOCKS + threadIdx.x] : 0.0, s_w);
    if (threadIdx.x != 0) return;
    double s[CL_SUMS];
    for (int c = 0; c < CL_SUMS; ++c) {
        s[c] = 0.0;
        for (int b = 0; b < B; ++b) s[c] += sums[((size_t)task * B + b) * CL_SUMS + c];
    }
    const int np = num_pos[task];
    const double hm_loss = np > 0 ? -(s[0] + n) / (double)np : -n;
    float* o = out + task * 14;
    double loc = 0.0;
    for (int c = 0; c < 10; ++c) {
        const double e = s[1 + c] / ((double)np + 1e-4);
        o[3 + c] = (float)e;
        loc += e * (double)cw.w[c];
    }
    o[0] = (float)(hm_loss + (double)weight * loc);
    o[1] = (float)hm_loss;
    o[2] = (float)loc;
    o[13] = (float)np;
}

}  // namespace shasta

using namespace shasta;

extern "C" size_t shasta_center_loss_workspace_bytes(int num_tasks, int B) {
    if (!cl_sizes_ok(num_tasks, B)) return 0;
    return ClWs(nullptr, num_tasks, B).bytes;
}

extern "C" int shasta_center_loss_f32(const shasta_center_loss_task* h_tasks, int num_tasks, int B, int H, int W, int max_objs, float weight,
                                      const float* h_code_weights, float* out, void* workspace, size_t workspace_bytes,
                                      shasta_stream_t stream) {
    SHASTA_REQUIRE(h_tasks && h_code_weights && out && workspace, "center loss: null pointer");
    if (!cl_sizes_ok(num_tasks, B) || H < 1 || H > SHASTA_CENTER_MAX_MAP || W < 1 || W > SHASTA_CENTER_MAX_MAP || max_objs < 1 ||
        max_objs > SHASTA_CENTER_MAX_OBJS) {
        set_error_msg("center loss: 1..16 tasks, 1..64 samples, 1..1024 objects per task, maps up to 512 x 512");
        return SHASTA_E_UNSUPPORTED;
    }
    const int HW = H * W;
    ClTable tab = {};
    for (int t = 0; t < num_tasks; ++t) {
        const shasta_center_loss_task& K = h_tasks[t];
        if (K.num_class < 1 || K.num_class > SHASTA_CENTER_MAX_TASK_CLASSES) {
            set_error_msg("center loss: 1..4 classes per task");
            return SHASTA_E_UNSUPPORTED;
        }
        SHASTA_REQUIRE(K.hm && K.target_hm && K.anno_box && K.ind && K.cat && K.mask && K.g_hm && K.g_box, "center loss: null tensor in a task");
        SHASTA_REQUIRE(K.hm_stride >= (int64_t)K.num_class * HW, "center loss: a sample stride below the sample's size");
        const int width[5] = {2, 1, 3, 2, 2};
        for (int i = 0; i < 5; ++i) {
            SHASTA_REQUIRE(K.box[i], "center loss: null box head in a task");
            SHASTA_REQUIRE(K.box_stride[i] >= (int64_t)width[i] * HW, "center loss: a sample stride below the sample's size");
        }
        tab.t[t] = K;
    }
    if ((uintptr_t)workspace % 16) {
        set_error_msg("center loss: workspace must be 16-byte aligned");
        return SHASTA_E_ALIGN;
    }
    const ClWs L(workspace, num_tasks, B);
    if (workspace_bytes < L.bytes) {
        set_error_msg("center loss: workspace too small");
        return SHASTA_E_WORKSPACE;
    }
    ClCodeWeights cw;
    for (int c = 0; c < 10; ++c) cw.w[c] = h_code_weights[c];
    hipStream_t st = as_stream(stream);
    hipError_t e;
    for (int t = 0; t < num_tasks; ++t)
        if ((e = hipMemsetAsync(tab.t[t].g_box, 0, (size_t)B * 10 * HW * sizeof(float), st)) != hipSuccess) {
            set_error("center loss: memset", e);
            return SHASTA_E_LAUNCH;
        }
    int rc;
    hipLaunchKernelGGL(cl_count_kernel, dim3((unsigned)num_tasks), dim3(CL_THREADS), 0, st, tab, B * max_objs, L.num_pos);
    hipLaunchKernelGGL(cl_dense_kernel, dim3(CL_BLOCKS, (unsigned)num_tasks), dim3(CL_THREADS), 0, st, tab, B, HW, L.num_pos, L.neg);
    if ((rc = check_launch("cl_dense"))) return rc;
    hipLaunchKernelGGL(cl_sparse_kernel, dim3((unsigned)B, (unsigned)num_tasks), dim3(CL_THREADS), 0, st, tab, B, H, W, max_objs, weight, cw,
                       L.num_pos, L.sums);
    hipLaunchKernelGGL(cl_final_kernel, dim3((unsigned)num_tasks), dim3(CL_THREADS), 0, st, B, weight, cw, L.num_pos, L.neg, L.sums, out);
    return check_launch("cl_final");
}
