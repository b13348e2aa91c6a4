// fp32 "NT" GEMM on the bf16 matrix path:  C[m][n] = act(sum_k A[m][k] * W[n][k] + bias[n]),  A, W, C fp32.
// Same contract as gemm_nt_f32_kernel (gemm_f32.hip) for the nn.Linear layers that are applied to many table rows
// (det3d/models/tracker/shasta.py:59-67,86-92,94-106), but every fp32 product is formed from exact bf16 pieces: the six piece
// products of pieces.hpp.
// Workgroup = 4 waves = 128 x 128 output tile (each wave 64 x 64 = 2 x 2 accumulators of 32 x 32); K is walked in 32-wide
// slices: fp32 slices are prefetched into registers, cut on the VALU when they are stored to LDS (three bf16 images per
// operand, row stride 80 B so that the 16 lanes of a ds_read_b128 phase cover all 64 banks), and read back as MFMA
// fragments (8 consecutive k per lane).  Two workgroups per CU (60 KB of LDS each): one cuts while the other multiplies.
// (A one-workgroup-per-CU form with double-buffered LDS, one barrier per slice and the cut interleaved behind the MFMA chains
// of the same wave measured 61 us instead of 39.5 us on 64 256 x 128 x 256: the second workgroup hides more than the pipeline.)
// One problem per launch: the kernel serves the C entry shasta_gemm_nt_pieces_f32 only (tests, tools/time_gemm.py) - inside the
// forward embed_rows.hip took its place.
#include "gemm_tile.hpp"
#include "pieces.hpp"

namespace shasta {

constexpr int PM = 128, PN = 128, PK = 32;
constexpr int PROW = 80;                   // bytes per LDS row of one piece image: 32 bf16 + 16 B pad
constexpr int PIMG = PM * PROW;            // one piece image of one operand
static_assert(PM == PN, "both operands use the same staging code");

// 128 rows x 32 k of fp32 -> registers (4 float4 per thread); rows >= `rows` and k >= K read as zero
template <bool VEC>
__device__ __forceinline__ void pieces_load(const float* __restrict__ P, int ld, int rows, int K, int r0, int k0, int tid,
                                            f32x4 (&reg)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i;
        const int gr = r0 + (idx >> 3), gk = k0 + 4 * (idx & 7);
        if (VEC && gr < rows && gk + 3 < K) {
            reg[i] = *reinterpret_cast<const f32x4*>(P + (size_t)gr * ld + gk);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) reg[i][j] = (gr < rows && gk + j < K) ? P[(size_t)gr * ld + gk + j] : 0.0f;
        }
    }
}

// registers -> three bf16 images in LDS
__device__ __forceinline__ void pieces_store(char* img, int tid, const f32x4 (&reg)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i;
        char* dst = img + (idx >> 3) * PROW + (idx & 7) * 8;
        float h[4], m[4], l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) cut3_bf16(reg[i][j], h[j], m[j], l[j]);
        *reinterpret_cast<u32x2*>(dst) = u32x2{pack_bf16x2(h[0], h[1]), pack_bf16x2(h[2], h[3])};
        *reinterpret_cast<u32x2*>(dst + PIMG) = u32x2{pack_bf16x2(m[0], m[1]), pack_bf16x2(m[2], m[3])};
        *reinterpret_cast<u32x2*>(dst + 2 * PIMG) = u32x2{pack_bf16x2(l[0], l[1]), pack_bf16x2(l[2], l[3])};
    }
}

struct GemmPieces {
    GemmNtSet<1> p;
    int lda, ldw, ldc, M, N, K, act;
};

template <bool VEC>
__global__ __launch_bounds__(256) void gemm_nt_pieces_kernel(GemmPieces g) {
    __shared__ __attribute__((aligned(16))) char s_a[3 * PIMG];
    __shared__ __attribute__((aligned(16))) char s_w[3 * PIMG];
    const float* __restrict__ A = g.p.A[0];
    const float* __restrict__ W = g.p.W[0];
    const float* __restrict__ bias = g.p.bias[0];
    float* __restrict__ C = g.p.C[0];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int m0 = blockIdx.y * PM, n0 = blockIdx.x * PN;
    f32x4 ra[4], rw[4];
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int nk = (g.K + PK - 1) / PK;
    pieces_load<VEC>(A, g.lda, g.M, g.K, m0, 0, tid, ra);
    pieces_load<VEC>(W, g.ldw, g.N, g.K, n0, 0, tid, rw);
    // fragment of row-block i, k-step s, piece p: 8 consecutive k of row 64*w + 32*i + (lane & 31), k = 16 s + 8 (lane >> 5)
    const char* af = s_a + (wm * 64 + (lane & 31)) * PROW + (lane >> 5) * 16;
    const char* wf = s_w + (wn * 64 + (lane & 31)) * PROW + (lane >> 5) * 16;
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();  // previous slice fully consumed
        pieces_store(s_a, tid, ra);
        pieces_store(s_w, tid, rw);
        __syncthreads();
        if (kt + 1 < nk) {
            pieces_load<VEC>(A, g.lda, g.M, g.K, m0, (kt + 1) * PK, tid, ra);
            pieces_load<VEC>(W, g.ldw, g.N, g.K, n0, (kt + 1) * PK, tid, rw);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            u32x4 fa[2][3], fw[2][3];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    fa[i][p] = *reinterpret_cast<const u32x4*>(af + p * PIMG + i * 32 * PROW + s * 32);
                    fw[i][p] = *reinterpret_cast<const u32x4*>(wf + p * PIMG + i * 32 * PROW + s * 32);
                }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int q = 0; q < 6; ++q)
                        acc[i][j] = mfma_32x32x16_bf16(fa[i][kProductsBf16[q].a], fw[j][kProductsBf16[q].b], acc[i][j]);
        }
    }
    // C/D map of a 32x32 accumulator: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn * 64 + 32 * j + (lane & 31);
        if (col >= g.N) continue;
        const float bv = bias ? bias[col] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * 64 + 32 * i + mfma32_row(r, lane >> 5);
                if (row < g.M) C[(size_t)row * g.ldc + col] = gemm_act(acc[i][j][r] + bv, g.act);
            }
    }
}

static int launch_gemm_nt_pieces(const float* A, const float* W, const float* bias, float* C, int lda, int ldw, int ldc, int M, int N, int K,
                                 int act, hipStream_t st) {
    if (M == 0 || N == 0) return SHASTA_OK;
    GemmPieces g{{{A}, {W}, {bias}, {C}}, lda, ldw, ldc, M, N, K, act};
    dim3 grid(cdiv(N, PN), cdiv(M, PM));
    if (gemm_vec_ok(lda, ldw, A, W)) hipLaunchKernelGGL(gemm_nt_pieces_kernel<true>, grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL(gemm_nt_pieces_kernel<false>, grid, dim3(256), 0, st, g);
    return check_launch("gemm_nt_pieces");
}

}  // namespace shasta

extern "C" int shasta_gemm_nt_pieces_f32(const float* A, int lda, const float* W, int ldw, const float* bias, float* C,
                                         int ldc, int M, int N, int K, int act, shasta_stream_t stream) {
    using namespace shasta;
    SHASTA_REQUIRE(A && W && C, "gemm_nt_pieces: null pointer");
    SHASTA_REQUIRE(M >= 0 && N >= 0 && K > 0 && lda >= K && ldw >= K && ldc >= N, "gemm_nt_pieces: bad size");
    SHASTA_REQUIRE(act >= 0 && act <= 2, "gemm_nt_pieces: bad activation");
    return launch_gemm_nt_pieces(A, W, bias, C, lda, ldw, ldc, M, N, K, act, as_stream(stream));
}
