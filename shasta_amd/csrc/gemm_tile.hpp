// What the dense GEMM kernels of gemm_f32.hip and gemm_pieces.hip share: the problem set of a multi-problem launch, the activation of
// their epilogues and the host-side precondition of their 16-byte operand loads.
#pragma once
#include "common.hpp"

namespace shasta {

// N independent NT problems of one shape in one launch (blockIdx.z picks the problem)
template <int N>
struct GemmNtSet {
    const float* A[N];
    const float* W[N];
    const float* bias[N];
    float* C[N];
};

// act: 0 none, 1 ReLU, 2 |.|
__device__ __forceinline__ float gemm_act(float v, int act) {
    if (act == 1) v = relu_nan(v);
    else if (act == 2) v = fabsf(v);
    return v;
}

// one dwordx4 load per 4 k of a row: leading dimensions in multiples of 4 floats, 16-byte aligned operands
template <class... P>
inline bool gemm_vec_ok(int lda, int ldw, const P*... operands) {
    return lda % 4 == 0 && ldw % 4 == 0 && ((... | (uintptr_t)operands) % 16 == 0);
}

}  // namespace shasta
