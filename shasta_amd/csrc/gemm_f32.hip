// Generic fp32 "NT" GEMM on the CDNA4 matrix cores:  C[m][n] = act(sum_k A[m][k] * W[n][k] + bias[n])
// Both operands are K-contiguous (activations row major, nn.Linear weight (out,in) row major), so this
// is the one dense kernel behind every nn.Linear of the path that is applied to many rows:
//   * the factorised first layers of fuse_shape / res_coeff (shasta.py:59-67,86-92) on the T+D table rows,
//   * the six aff layers (shasta.py:94-106) on the B*T residual rows.
// v_mfma_f32_32x32x2_f32: f32 in / f32 accumulate, bit-for-bit a k-ordered fmaf chain (exact fp32; gfx950 has
// no xf32), 64 FLOP/clk/SIMD.  Workgroup = 4 waves = 64x64 output tile, each wave one 32x32 accumulator
// (16 VGPRs); K is walked in 32-wide slices staged through LDS (row stride 33 floats: the one-float-per-lane
// fragment reads A[i=l&31][k=l>>5] then hit 32 distinct banks), next slice prefetched into registers while
// the current one is multiplied.
// Layout of this file: how a slice lies in LDS (OperandF32 / OperandBf16), the two kinds of global operand with their loaders, and
// gemm_tile, the one 64 x 64 tile with its K walk that the NT and the strided kernels instantiate; the NT kernels, wave_sum_epilogue
// with the two kernels that split K over the waves, and the NT launchers; then the strided form of the training path: its kernels,
// plan_gemm_strided (the one split-K decision) and the single and the group launcher.
#include "gemm_tile.hpp"
#include "stages.hpp"

namespace shasta {

constexpr int BM = 64, BN = 64, BK = 32;
constexpr int LDS_LD = BK + 1;  // f32 LDS rows (above)
// bf16 LDS rows are 32 + 8 bf16 = 80 bytes: the 16 lanes of a ds_read_b128 phase start 20 banks apart and cover all 64 banks
constexpr int LDH = BK + 8;

__device__ __forceinline__ uint16_t to_bf16_bits(float v) { return __builtin_bit_cast(uint16_t, (__bf16)v); }

// How an operand slice lies in LDS and goes to the matrix cores: element type, row stride, the lane's k offset inside a row (lanes
// 32 - 63 hold the second k / the second 8 k of an MFMA step), the store of a 64 x 32 slice from the loaders' registers and the MFMA chain
// over one slice.  store: (s_r, s_k) are the operand's strides - k-contiguous or general operands were loaded as thread -> (row, 4
// consecutive k), row-contiguous ones as element e = (i*4 + j)*256 + tid of the tile, row = e & 63, k = e >> 6.
struct OperandF32 {
    typedef float elem;
    static constexpr int LD = LDS_LD, LANE_K = 1;
    static __device__ __forceinline__ void store(float* S, long s_r, long s_k, int tid, const float (&reg)[2][4]) {
        if (s_k == 1 || s_r != 1) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int idx = tid + 256 * i;
                const int row = idx >> 3, c4 = idx & 7;
#pragma unroll
                for (int j = 0; j < 4; ++j) S[row * LDS_LD + 4 * c4 + j] = reg[i][j];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = (i * 4 + j) * 256 + tid;
                    S[(e & 63) * LDS_LD + (e >> 6)] = reg[i][j];
                }
        }
    }
    static __device__ __forceinline__ f32x16 chain(const float* af, const float* wf, f32x16 acc) {
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[2 * s], wf[2 * s], acc, 0, 0, 0);
        return acc;
    }
};
// bf16 operands (act & 8 of the strided form; BASELINE config 5's reduced-precision option for the training GEMMs): the fp32 operands
// in HBM are rounded to bf16 (nearest even) when a K slice is stored to LDS and multiplied on v_mfma_f32_32x32x16_bf16 with fp32
// accumulation - master weights, activations in HBM, bias / activation epilogue and the split-K sums all stay fp32.
struct OperandBf16 {
    typedef uint16_t elem;
    static constexpr int LD = LDH, LANE_K = 8;
    static __device__ __forceinline__ void store(uint16_t* S, long s_r, long s_k, int tid, const float (&reg)[2][4]) {
        if (s_k == 1 || s_r != 1) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int idx = tid + 256 * i;
                const int row = idx >> 3, c4 = idx & 7;
                uint32_t* d = reinterpret_cast<uint32_t*>(S + row * LDH + 4 * c4);
                d[0] = (uint32_t)to_bf16_bits(reg[i][0]) | ((uint32_t)to_bf16_bits(reg[i][1]) << 16);
                d[1] = (uint32_t)to_bf16_bits(reg[i][2]) | ((uint32_t)to_bf16_bits(reg[i][3]) << 16);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = (i * 4 + j) * 256 + tid;
                    S[(e & 63) * LDH + (e >> 6)] = to_bf16_bits(reg[i][j]);
                }
        }
    }
    static __device__ __forceinline__ f32x16 chain(const uint16_t* af, const uint16_t* wf, f32x16 acc) {
#pragma unroll
        for (int s = 0; s < BK / 16; ++s) {
            const u32x4 a = *reinterpret_cast<const u32x4*>(af + 16 * s), w = *reinterpret_cast<const u32x4*>(wf + 16 * s);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, w), acc, 0, 0, 0);
        }
        return acc;
    }
};

// The two kinds of global-memory operand.  Each describes itself as {P, s_r, s_k, rows, vec} - element (r, k) at P[r * s_r + k * s_k] -
// and has a load_slice overload that fetches the 64 x 32 slice at (r0, k0) into registers, 8 floats per thread; rows >= `rows` and
// k >= K read as zero.  (Two loaders, not one: int against long strides, and the NT form knows its layout at compile time.)
// NT form: rows of s_r floats, k-contiguous; VEC: one dwordx4 load per 4 k (gemm_vec_ok)
template <bool VEC>
struct VecLoads {};
template <bool VEC>
struct NtOperand {
    const float* P;
    int s_r, rows;
    static constexpr long s_k = 1;
    static constexpr VecLoads<VEC> vec = {};
};
template <bool VEC>
__device__ __forceinline__ void load_slice(const float* __restrict__ P, int ld, long, int rows, VecLoads<VEC>, int K, int r0, int k0, int tid,
                                           float (&reg)[2][4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i;
        const int row = idx >> 3, c4 = idx & 7;
        const int gr = r0 + row, gk = k0 + 4 * c4;
        if (VEC && gr < rows && gk + 3 < K) {
            const float4 v = *reinterpret_cast<const float4*>(P + (size_t)gr * ld + gk);
            reg[i][0] = v.x; reg[i][1] = v.y; reg[i][2] = v.z; reg[i][3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                reg[i][j] = (gr < rows && gk + j < K) ? P[(size_t)gr * ld + gk + j] : 0.0f;
        }
    }
}

// strided form (training path, below): any strides; vec: k-contiguous rows, 16-byte aligned (strided_vec_ok)
struct StridedOperand {
    const float* P;
    long s_r, s_k;
    int rows;
    bool vec;
};
__device__ __forceinline__ void load_slice(const float* __restrict__ P, long s_r, long s_k, int rows, bool vec, int K, int r0, int k0, int tid,
                                           float (&reg)[2][4]) {
    if (s_k == 1 || s_r != 1) {  // k-contiguous (or general): thread -> (row, 4 consecutive k)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx >> 3, c4 = idx & 7;
            const int gr = r0 + row, gk = k0 + 4 * c4;
            if (vec && gr < rows && gk + 3 < K) {  // k-contiguous, 16-byte aligned rows: one dwordx4 load
                const f32x4 v = *reinterpret_cast<const f32x4*>(P + (long)gr * s_r + gk);
#pragma unroll
                for (int j = 0; j < 4; ++j) reg[i][j] = v[j];
                continue;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) reg[i][j] = (gr < rows && gk + j < K) ? P[(long)gr * s_r + (long)(gk + j) * s_k] : 0.0f;
        }
    } else {  // row-contiguous: adjacent threads read adjacent rows of the same k (coalesced)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // element e = (i*4 + j)*256 + tid of the 64 x 32 tile: row = e & 63, k = e >> 6
                const int e = (i * 4 + j) * 256 + tid;
                const int row = e & 63, kk = e >> 6;
                const int gr = r0 + row, gk = k0 + kk;
                reg[i][j] = (gr < rows && gk < K) ? P[(long)gr + (long)gk * s_k] : 0.0f;
            }
    }
}

// One 64 x 64 output tile of every kernel of this file that stages its operands through LDS.  `Tile` is the problem: its operands a()
// and w(), the reduction range of this workgroup and the epilogue; `Op` how a slice lies in LDS.  K is walked in slices of 32: the next
// slice is prefetched into registers while the current one is multiplied.  MAY_BE_EMPTY: the range can be empty (the strided form with
// K = 0), so the first load is guarded as well.
// (The loaders are called right here with scalar arguments, the operand pointer as their own __restrict__ parameter, and the operand
// descriptions are asked for at every use: a loader behind a lambda, a functor or a description passed by reference, or descriptions
// copied once at the top, all compile to other instruction streams for the strided kernels than the hand-written loop did.)
#define GEMM_OPERAND(o) (o).P, (o).s_r, (o).s_k, (o).rows, (o).vec
template <class Op, bool MAY_BE_EMPTY, class Tile>
__device__ __forceinline__ void gemm_tile(const Tile& t, int by) {
    __shared__ __attribute__((aligned(16))) typename Op::elem As[BM * Op::LD];
    __shared__ __attribute__((aligned(16))) typename Op::elem Ws[BN * Op::LD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int m0 = by * BM, n0 = blockIdx.x * BN;
    int kbeg, kend;
    t.k_range(kbeg, kend);
    float ra[2][4], rw[2][4];
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int nk = (kend - kbeg + BK - 1) / BK;
    if (!MAY_BE_EMPTY || nk > 0) {
        load_slice(GEMM_OPERAND(t.a()), kend, m0, kbeg, tid, ra);
        load_slice(GEMM_OPERAND(t.w()), kend, n0, kbeg, tid, rw);
    }
    const typename Op::elem* af = As + (wm * 32 + (lane & 31)) * Op::LD + (lane >> 5) * Op::LANE_K;
    const typename Op::elem* wf = Ws + (wn * 32 + (lane & 31)) * Op::LD + (lane >> 5) * Op::LANE_K;
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();  // previous slice fully consumed
        Op::store(As, t.a().s_r, t.a().s_k, tid, ra);
        Op::store(Ws, t.w().s_r, t.w().s_k, tid, rw);
        __syncthreads();
        if (kt + 1 < nk) {
            load_slice(GEMM_OPERAND(t.a()), kend, m0, kbeg + (kt + 1) * BK, tid, ra);
            load_slice(GEMM_OPERAND(t.w()), kend, n0, kbeg + (kt + 1) * BK, tid, rw);
        }
        acc = Op::chain(af, wf, acc);
    }
    t.epilogue(acc, m0, n0, wm, wn, lane);
}
#undef GEMM_OPERAND

// the NT problem: the whole K in one workgroup (K > 0), bias and activation as the epilogue
template <bool VEC>
struct NtTile {
    NtOperand<VEC> a_, w_;  // (M, K) and (N, K)
    const float* __restrict__ bias;
    float* __restrict__ C;
    int ldc, K, act;
    __device__ __forceinline__ const NtOperand<VEC>& a() const { return a_; }
    __device__ __forceinline__ const NtOperand<VEC>& w() const { return w_; }
    __device__ __forceinline__ void k_range(int& kbeg, int& kend) const {
        kbeg = 0;
        kend = K;
    }
    // C/D map of the 32x32 accumulator: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
    __device__ __forceinline__ void epilogue(const f32x16& acc, int m0, int n0, int wm, int wn, int lane) const {
        const int col = n0 + wn * 32 + (lane & 31);
        if (col < w_.rows) {
            const float bv = bias ? bias[col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * 32 + mfma32_row(r, lane >> 5);
                if (row < a_.rows) C[(size_t)row * ldc + col] = gemm_act(acc[r] + bv, act);
            }
        }
    }
};
template <bool VEC>
__device__ __forceinline__ void gemm_nt_tile(const float* __restrict__ A, int lda, const float* __restrict__ W, int ldw,
                                             const float* __restrict__ bias, float* __restrict__ C, int ldc, int M, int N, int K, int act) {
    gemm_tile<OperandF32, false>(NtTile<VEC>{{A, lda, M}, {W, ldw, N}, bias, C, ldc, K, act}, blockIdx.y);
}

template <bool VEC>
__global__ __launch_bounds__(256) void gemm_nt_f32_kernel(const float* __restrict__ A, int lda,
                                                          const float* __restrict__ W, int ldw,
                                                          const float* __restrict__ bias, float* __restrict__ C,
                                                          int ldc, int M, int N, int K, int act) {
    gemm_nt_tile<VEC>(A, lda, W, ldw, bias, C, ldc, M, N, K, act);
}

// two independent problems of the same shape in one launch (blockIdx.z picks the problem): the two row-embedding GEMMs of
// the pair stage are small (16 workgroups each at one frame pair), one launch runs them side by side
__global__ __launch_bounds__(256) void gemm_nt_f32_dual_kernel(GemmNtSet<2> p, int lda, int ldw, int ldc, int M, int N, int K, int act) {
    const int z = blockIdx.z;
    gemm_nt_tile<true>(z ? p.A[1] : p.A[0], lda, z ? p.W[1] : p.W[0], ldw, z ? p.bias[1] : p.bias[0], z ? p.C[1] : p.C[0], ldc, M, N, K, act);
}

// up to four independent problems of one shape in one launch (blockIdx.z picks the problem): the second layers of the four
// aug_shape / first layers of the four aug_dets anchor MLPs at batch >= 16 (anchor.hip)
template <bool VEC>
__global__ __launch_bounds__(256) void gemm_nt_f32_quad_kernel(GemmNtSet<4> p, int lda, int ldw, int ldc, int M, int N, int K, int act) {
    const int z = blockIdx.z;
    gemm_nt_tile<VEC>(p.A[z], lda, p.W[z], ldw, p.bias[z], p.C[z], ldc, M, N, K, act);
}

// The four waves of a workgroup hold one partial sum each of a 32 x 32 tile (a share of K per wave): added in wave order through LDS,
// then bias, activation and the store.  Accumulator map: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ void wave_sum_epilogue(const f32x16& acc, const float* bias, float* C, int ldc, int M, int N, int m0, int n0,
                                                  int act, int tid, int wid, int r, int h) {
    __shared__ float red[4][32][33];
#pragma unroll
    for (int q = 0; q < 16; ++q) red[wid][(q & 3) + 8 * (q >> 2) + 4 * h][r] = acc[q];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = tid + 256 * i, row = e >> 5, col = e & 31;
        if (m0 + row < M && n0 + col < N) {
            float v = ((red[0][row][col] + red[1][row][col]) + red[2][row][col]) + red[3][row][col];
            if (bias) v += bias[n0 + col];
            C[(size_t)(m0 + row) * ldc + n0 + col] = gemm_act(v, act);
        }
    }
}

// Few rows (the row embeddings of one or a few small frame-pairs: 12 workgroups of the kernel above walk ten dependent 32-wide slices,
// 13 us at max_obj 90, batch 1): the whole K in ONE round of loads.  A workgroup owns a 32 x 32 output tile; its four waves take a
// quarter of K each - every operand element of the wave straight from global memory into the MFMA layout, all loads in flight at
// once (lane (r, h) holds row r, elements [KQ/2 * h, KQ/2 * (h + 1)) of the wave's quarter for both operands, so MFMA step s pairs the
// same k on both sides) - and the four partial tiles are added in wave order through LDS.  K % 32 == 0 and K <= 512 (F = 64 .. 512).
template <int KQ>  // K / 4: elements per wave
__global__ __launch_bounds__(256) void gemm_nt_f32_small_dual_kernel(GemmNtSet<2> p, int lda, int ldw, int ldc, int M, int N, int act) {
    constexpr int KH = KQ / 2;  // elements per lane and operand
    static_assert(KH % 4 == 0, "16-byte loads");
    const int z = blockIdx.z;
    const float* A = z ? p.A[1] : p.A[0];
    const float* W = z ? p.W[1] : p.W[0];
    const float* bias = z ? p.bias[1] : p.bias[0];
    float* C = z ? p.C[1] : p.C[0];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const f32x4* ap = reinterpret_cast<const f32x4*>(A + (size_t)min(m0 + r, M - 1) * lda + wid * KQ + h * KH);
    const f32x4* wp = reinterpret_cast<const f32x4*>(W + (size_t)min(n0 + r, N - 1) * ldw + wid * KQ + h * KH);
    f32x4 av[KH / 4], wv[KH / 4];
#pragma unroll
    for (int i = 0; i < KH / 4; ++i) {
        av[i] = ap[i];
        wv[i] = wp[i];
    }
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < KH / 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][j], wv[i][j], acc, 0, 0, 0);
    wave_sum_epilogue(acc, bias, C, ldc, M, N, m0, n0, act, tid, wid, r, h);
}

// Skinny problems with a long K (the second aug_shape layers: M = batch, N = F, K = N F / 64; the first aug_dets layers: K = 7 N): the
// 64 x 64 tiles above are 16 .. 128 workgroups that walk K in 60 .. 110 dependent slices, 80 - 100 us whatever the batch.  Here a
// workgroup owns a 32 x 32 tile and walks K in chunks of 128: its four waves take 32 consecutive k of every chunk each, operands go
// straight from global memory (L2) into the MFMA layout - lane (r, h) holds row r, 16 consecutive k, for both operands -, the next
// chunk's loads are in flight under the 16 MFMAs of this one, no LDS and no barrier until the four partial tiles are added in wave
// order at the end.  Preconditions (gemm_nt_quad_direct_ok): K % 4 == 0, 16-byte aligned operand rows.  Measured at
// N = 500: 50 us against 94 us for the 64 x 64 tiles at 512 rows; at 64 rows 36 - 41 us, no better than the VALU kernels of the small
// batches (anchor.hip: 37 - 40 us), which therefore stay below 256 rows.
__global__ __launch_bounds__(256) void gemm_nt_f32_direct_quad_kernel(GemmNtSet<4> p, int lda, int ldw, int ldc, int M, int N, int K, int act) {
    const int z = blockIdx.z;
    const float* A = p.A[z];
    const float* W = p.W[z];
    const float* bias = p.bias[z];
    float* C = p.C[z];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const float* ap = A + (size_t)min(m0 + r, M - 1) * lda + wid * 32 + h * 16;
    const float* wp = W + (size_t)min(n0 + r, N - 1) * ldw + wid * 32 + h * 16;
    const int kl = wid * 32 + h * 16;  // this lane's first k inside a chunk
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    // (two chunks per wave in flight; four measured the same: 50.1 against 51.5 us at 512 rows, K = 2000 / 3500)
    constexpr int NB = 2;
    f32x4 av[NB][4], wv[NB][4];
    auto load = [&](int c, f32x4 (&a4)[4], f32x4 (&w4)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = c * 128 + kl + 4 * i < K;
            a4[i] = in ? *reinterpret_cast<const f32x4*>(ap + (size_t)c * 128 + 4 * i) : zero;
            w4[i] = in ? *reinterpret_cast<const f32x4*>(wp + (size_t)c * 128 + 4 * i) : zero;
        }
    };
    const int nc = (K + 127) / 128;
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < NB - 1; ++b)
        if (b < nc) load(b, av[b], wv[b]);
    for (int c = 0; c < nc; c += NB) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (c + b >= nc) break;
            if (c + b + NB - 1 < nc) load(c + b + NB - 1, av[(b + NB - 1) % NB], wv[(b + NB - 1) % NB]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[b][i][j], wv[b][i][j], acc, 0, 0, 0);
        }
    }
    wave_sum_epilogue(acc, bias, C, ldc, M, N, m0, n0, act, tid, wid, r, h);
}

static int launch_gemm_nt(const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc, int M,
                          int N, int K, int act, hipStream_t st) {
    if (M == 0 || N == 0) return SHASTA_OK;
    dim3 grid(cdiv(N, BN), cdiv(M, BM));
    if (gemm_vec_ok(lda, ldw, A, W))
        hipLaunchKernelGGL(gemm_nt_f32_kernel<true>, grid, dim3(256), 0, st, A, lda, W, ldw, bias, C, ldc, M, N, K, act);
    else
        hipLaunchKernelGGL(gemm_nt_f32_kernel<false>, grid, dim3(256), 0, st, A, lda, W, ldw, bias, C, ldc, M, N, K, act);
    return check_launch("gemm_nt_f32");
}

static bool quad_vec_ok(const float* const A[4], const float* const W[4], int lda, int ldw) {
    return gemm_vec_ok(lda, ldw, A[0], W[0], A[1], W[1], A[2], W[2], A[3], W[3]);
}
// true when launch_gemm_nt_quad will take the direct form for these operands
bool gemm_nt_quad_direct_ok(const float* const A[4], const float* const W[4], int lda, int ldw, int K) {
    return K % 4 == 0 && K >= 512 && quad_vec_ok(A, W, lda, ldw);
}
int launch_gemm_nt_quad(const float* const A[4], const float* const W[4], const float* const bias[4], float* const C[4], int lda,
                        int ldw, int ldc, int M, int N, int K, int act, hipStream_t st) {
    if (M == 0 || N == 0) return SHASTA_OK;
    GemmNtSet<4> p;
    for (int i = 0; i < 4; ++i) {
        p.A[i] = A[i];
        p.W[i] = W[i];
        p.bias[i] = bias[i];
        p.C[i] = C[i];
    }
    if (gemm_nt_quad_direct_ok(A, W, lda, ldw, K)) {  // skinny, long K: the direct form
        hipLaunchKernelGGL(gemm_nt_f32_direct_quad_kernel, dim3(cdiv(N, 32), cdiv(M, 32), 4), dim3(256), 0, st, p, lda, ldw, ldc, M, N, K, act);
        return check_launch("gemm_nt_f32_direct_quad");
    }
    dim3 grid(cdiv(N, BN), cdiv(M, BM), 4);
    if (quad_vec_ok(A, W, lda, ldw)) hipLaunchKernelGGL(gemm_nt_f32_quad_kernel<true>, grid, dim3(256), 0, st, p, lda, ldw, ldc, M, N, K, act);
    else hipLaunchKernelGGL(gemm_nt_f32_quad_kernel<false>, grid, dim3(256), 0, st, p, lda, ldw, ldc, M, N, K, act);
    return check_launch("gemm_nt_f32_quad");
}

// C0 = A0 W0^T (+bias0), C1 = A1 W1^T (+bias1), same shapes and leading dimensions; falls back to two launches when the
// vector-load preconditions do not hold
int launch_gemm_nt_dual(const float* A0, const float* W0, const float* bias0, float* C0, const float* A1, const float* W1,
                        const float* bias1, float* C1, int lda, int ldw, int ldc, int M, int N, int K, int act, hipStream_t st) {
    if (M == 0 || N == 0) return SHASTA_OK;
    if (!gemm_vec_ok(lda, ldw, A0, W0, A1, W1)) {
        int rc = launch_gemm_nt(A0, lda, W0, ldw, bias0, C0, ldc, M, N, K, act, st);
        if (rc) return rc;
        return launch_gemm_nt(A1, lda, W1, ldw, bias1, C1, ldc, M, N, K, act, st);
    }
    GemmNtSet<2> p{{A0, A1}, {W0, W1}, {bias0, bias1}, {C0, C1}};
    // while the 64 x 64 tiles leave most of the chip idle: the one-shot kernel (four times the workgroups, one load latency)
    if (2 * cdiv(N, BN) * cdiv(M, BM) <= 128 && (K == 64 || K == 256 || K == 320 || K == 512)) {
        const dim3 grid(cdiv(N, 32), cdiv(M, 32), 2);
        if (K == 64) hipLaunchKernelGGL(gemm_nt_f32_small_dual_kernel<16>, grid, dim3(256), 0, st, p, lda, ldw, ldc, M, N, act);
        else if (K == 256) hipLaunchKernelGGL(gemm_nt_f32_small_dual_kernel<64>, grid, dim3(256), 0, st, p, lda, ldw, ldc, M, N, act);
        else if (K == 320) hipLaunchKernelGGL(gemm_nt_f32_small_dual_kernel<80>, grid, dim3(256), 0, st, p, lda, ldw, ldc, M, N, act);
        else hipLaunchKernelGGL(gemm_nt_f32_small_dual_kernel<128>, grid, dim3(256), 0, st, p, lda, ldw, ldc, M, N, act);
        return check_launch("gemm_nt_f32_small_dual");
    }
    hipLaunchKernelGGL(gemm_nt_f32_dual_kernel, dim3(cdiv(N, BN), cdiv(M, BM), 2), dim3(256), 0, st, p, lda, ldw, ldc, M, N, K, act);
    return check_launch("gemm_nt_f32_dual");
}

}  // namespace shasta

extern "C" int shasta_gemm_nt_f32(const float* A, int lda, const float* W, int ldw, const float* bias, float* C,
                                  int ldc, int M, int N, int K, int act, shasta_stream_t stream) {
    using namespace shasta;
    SHASTA_REQUIRE(A && W && C, "gemm_nt: null pointer");
    SHASTA_REQUIRE(M >= 0 && N >= 0 && K > 0 && lda >= K && ldw >= K && ldc >= N, "gemm_nt: bad size");
    SHASTA_REQUIRE(act >= 0 && act <= 2, "gemm_nt: bad activation");
    return launch_gemm_nt(A, lda, W, ldw, bias, C, ldc, M, N, K, act, as_stream(stream));
}

namespace shasta {

// ------------------------------------------------------------------------------------------------------------------
// Strided form for the training path (backward of every nn.Linear):
//   C[m][n] (+)= sum_k A(m, k) * W(n, k),  A(m, k) = A[m*sa_m + k*sa_k], W(n, k) = W[n*sw_n + k*sw_k]
//   forward  Y  = X . W^T        : sa = (ldx, 1),  sw = (ldw, 1)           (the NT kernel above)
//   dX = dY . W                  : A = dY (ldy, 1), "W" = W^T  -> sw = (1, ldw)          reduction over out features
//   dW = dY^T . X                : A = dY^T -> sa = (1, ldy), "W" = X^T -> sw = (1, ldx)  reduction over rows
// Optional epilogue: bias, activation, and a ReLU mask (C *= mask > 0) for the backward through a ReLU.
// Split-K (grid.z slices of the reduction) writes partial tiles to `C + z*slice_stride`; the caller sums them in a fixed
// order (gemm_reduce_kernel) -> deterministic, no float atomics.
// ------------------------------------------------------------------------------------------------------------------
struct GemmS {
    const float* A;
    const float* W;
    const float* bias;
    const float* mask;  // (M, ldmask) or nullptr
    float* C;
    long sa_m, sa_k, sw_n, sw_k;
    int vec_a, vec_w;  // operand rows are k-contiguous and 16-byte aligned: vector loads
    int ldc, ldmask, M, N, K, act, kslice;  // kslice: reduction elements per grid.z slice (multiple of BK); act & 4: C += result
    long slice_stride;
};

// A GROUP of up to 8 products of one shape (the four aug_shape / aug_dets MLPs of the anchor backward, the two sides of a pair MLP's
// first layer): operands, bias, mask and result per member, everything else shared; grid.y = members x row tiles.  Each member is
// computed exactly as a launch of its own would (same tiles, same reduction slices): the group saves launches, not arithmetic.
constexpr int GEMM_GROUP_MAX = 8;
struct GemmGroup {
    const float* A[GEMM_GROUP_MAX];
    const float* W[GEMM_GROUP_MAX];
    const float* bias[GEMM_GROUP_MAX];
    const float* mask[GEMM_GROUP_MAX];
    float* C[GEMM_GROUP_MAX];
    int mtiles;  // row tiles per member
};
__device__ __forceinline__ GemmS group_member(const GemmS& g0, const GemmGroup& gg, int& by) {
    GemmS g = g0;
    const int m = blockIdx.y / gg.mtiles;
    by = blockIdx.y - m * gg.mtiles;
    g.A = gg.A[m];
    g.W = gg.W[m];
    g.bias = gg.bias[m];
    g.mask = gg.mask[m];
    g.C = gg.C[m];
    return g;
}

// epilogue of the strided kernels: bias, activation, ReLU mask, accumulate
// (a function of its own: written out inside StridedTile::epilogue it compiles to another instruction stream)
__device__ __forceinline__ void strided_epilogue(const GemmS& g, const f32x16& acc, int m0, int n0, int wm, int wn, int lane) {
    float* C = g.C + (long)blockIdx.z * g.slice_stride;
    const int col = n0 + wn * 32 + (lane & 31);
    if (col < g.N) {
        const float bv = (g.bias && blockIdx.z == 0) ? g.bias[col] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + wm * 32 + mfma32_row(r, lane >> 5);
            if (row < g.M) {
                float v = gemm_act(acc[r] + bv, g.act & 3);
                if (g.mask && !(g.mask[(long)row * g.ldmask + col] > 0.0f)) v = 0.0f;
                if (g.act & 4) v += C[(long)row * g.ldc + col];
                C[(long)row * g.ldc + col] = v;
            }
        }
    }
}

// the strided problem: reduction slice blockIdx.z of the product `g`
struct StridedTile {
    const GemmS& g;
    __device__ __forceinline__ StridedOperand a() const { return {g.A, g.sa_m, g.sa_k, g.M, g.vec_a != 0}; }
    __device__ __forceinline__ StridedOperand w() const { return {g.W, g.sw_n, g.sw_k, g.N, g.vec_w != 0}; }
    __device__ __forceinline__ void k_range(int& kbeg, int& kend) const {
        kbeg = blockIdx.z * g.kslice;
        kend = min(g.K, kbeg + g.kslice);
    }
    __device__ __forceinline__ void epilogue(const f32x16& acc, int m0, int n0, int wm, int wn, int lane) const {
        strided_epilogue(g, acc, m0, n0, wm, wn, lane);
    }
};
__global__ __launch_bounds__(256) void gemm_strided_f32_kernel(GemmS g) { gemm_tile<OperandF32, true>(StridedTile{g}, blockIdx.y); }
__global__ __launch_bounds__(256) void gemm_strided_bf16_kernel(GemmS g) { gemm_tile<OperandBf16, true>(StridedTile{g}, blockIdx.y); }
__global__ __launch_bounds__(256) void gemm_strided_group_f32_kernel(GemmS g0, GemmGroup gg) {
    int by;
    const GemmS g = group_member(g0, gg, by);
    gemm_tile<OperandF32, true>(StridedTile{g}, by);
}
__global__ __launch_bounds__(256) void gemm_strided_group_bf16_kernel(GemmS g0, GemmGroup gg) {
    int by;
    const GemmS g = group_member(g0, gg, by);
    gemm_tile<OperandBf16, true>(StridedTile{g}, by);
}

// C[row][col] = sum_z part[z*stride + i], i = row*N + col: 16 elements x 16 z-groups per block, each group sums its
// slices in order and the groups are combined in order (fixed association -> deterministic)
__device__ __forceinline__ void gemm_reduce_body(const float* __restrict__ part, long stride, int nz, float* __restrict__ C, long n, int N,
                                                 int ldc, const float* __restrict__ bias, int act) {
    __shared__ float red[16][17];
    const int e = threadIdx.x & 15, q = threadIdx.x >> 4;
    const long i = (long)blockIdx.x * 16 + e;
    float s = 0.0f;
    if (i < n)
        for (int z = q; z < nz; z += 16) s += part[(long)z * stride + i];
    red[q][e] = s;
    __syncthreads();
    if (q == 0 && i < n) {
        float t = red[0][e];
#pragma unroll
        for (int k = 1; k < 16; ++k) t += red[k][e];
        if (bias) t += bias[i % N];
        C[(i / N) * ldc + (i % N)] = gemm_act(t, act & 3);
    }
}
__global__ __launch_bounds__(256) void gemm_reduce_kernel(const float* __restrict__ part, long stride, int nz, float* __restrict__ C,
                                                          long n, int N, int ldc, const float* __restrict__ bias, int act) {
    gemm_reduce_body(part, stride, nz, C, n, N, ldc, bias, act);
}
// grid.y = member: its slices lie nz * stride apart in `part`
__global__ __launch_bounds__(256) void gemm_reduce_group_kernel(const float* __restrict__ part, long stride, int nz, GemmGroup gg, long n, int N,
                                                                int ldc, int act) {
    gemm_reduce_body(part + (size_t)blockIdx.y * nz * stride, stride, nz, gg.C[blockIdx.y], n, N, ldc, gg.bias[blockIdx.y], act);
}

// How one product (a launch of its own or a group member) walks its reduction: `nz` grid.z slices of `kslice` elements; with more than
// one slice the kernel writes partial tiles `slice_stride` apart into the scratch and a reduce kernel sums them.
// Long reductions with few output tiles (weight gradients) are split (bias and activation then belong to the sum of the slices: the
// reduce kernel applies them) - from K = 256 in slices of at least 128: a few-row GEMM with K = 450 ... 630 in ONE workgroup took
// 30 - 36 us of the car configuration's training step, four times per step.  `scratch_bytes`: what this product may use (0: none).
struct GemmStridedPlan {
    int nz, kslice;
    long slice_stride;  // 0: one slice, straight into C
};
static GemmStridedPlan plan_gemm_strided(int M, int N, int K, int act, bool any_mask, size_t scratch_bytes) {
    const int tiles = cdiv(M, BM) * cdiv(N, BN);
    int nz = 1;
    if (K >= 256 && tiles < 128 && !any_mask && (act & 4) == 0) {
        nz = min(min(512, cdiv(1024, tiles)), cdiv(K, 128));
        while (nz > 1 && (size_t)nz * M * N * sizeof(float) > scratch_bytes) --nz;
    }
    if (nz <= 1) return {1, cdiv(max(K, 1), BK) * BK, 0};
    const int kslice = cdiv(cdiv(K, nz), BK) * BK;
    return {cdiv(K, kslice), kslice, (long)M * N};
}

// the GemmS of a launch but for its five pointers; split-K: partial tiles (M, N), no epilogue but the operand precision
static GemmS gemm_strided_args(const GemmStridedPlan& p, long sa_m, long sa_k, long sw_n, long sw_k, bool vec_a, bool vec_w, int ldmask,
                               int ldc, int M, int N, int K, int act) {
    GemmS g = {};
    g.sa_m = sa_m; g.sa_k = sa_k; g.sw_n = sw_n; g.sw_k = sw_k;
    g.vec_a = vec_a ? 1 : 0;
    g.vec_w = vec_w ? 1 : 0;
    g.ldmask = ldmask; g.M = M; g.N = N; g.K = K;
    g.ldc = p.slice_stride ? N : ldc;
    g.act = p.slice_stride ? act & 8 : act;
    g.kslice = p.kslice;
    g.slice_stride = p.slice_stride;
    return g;
}
// vector loads of a strided operand: k-contiguous rows, 16-byte aligned
static bool strided_vec_ok(long s_r, long s_k, const float* P) { return s_k == 1 && s_r % 4 == 0 && ((uintptr_t)P & 15) == 0; }

static int launch_gemm_strided(const float* A, long sa_m, long sa_k, const float* W, long sw_n, long sw_k, const float* bias,
                               const float* mask, int ldmask, float* C, int ldc, int M, int N, int K, int act, float* splitk_ws,
                               size_t splitk_ws_bytes, hipStream_t st) {
    if (M == 0 || N == 0) return SHASTA_OK;
    const GemmStridedPlan p = plan_gemm_strided(M, N, K, act, mask != nullptr, splitk_ws ? splitk_ws_bytes : 0);
    const bool split = p.slice_stride != 0;
    GemmS g = gemm_strided_args(p, sa_m, sa_k, sw_n, sw_k, strided_vec_ok(sa_m, sa_k, A), strided_vec_ok(sw_n, sw_k, W), ldmask, ldc, M, N, K, act);
    g.A = A; g.W = W; g.mask = mask;
    g.bias = split ? nullptr : bias;
    g.C = split ? splitk_ws : C;
    const dim3 grid(cdiv(N, BN), cdiv(M, BM), p.nz);
    if (act & 8) hipLaunchKernelGGL(gemm_strided_bf16_kernel, grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL(gemm_strided_f32_kernel, grid, dim3(256), 0, st, g);
    int rc = check_launch(split ? "gemm_strided(split-K)" : "gemm_strided");
    if (rc || !split) return rc;
    const long n = (long)M * N;
    hipLaunchKernelGGL(gemm_reduce_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, splitk_ws, p.slice_stride, p.nz, C, n, N, ldc, bias, act);
    return check_launch("gemm_reduce");
}

// `count` products of one shape in one launch (two with a split reduction); every member as launch_gemm_strided would compute it alone
// when given count-th of the scratch: the same plan
static int launch_gemm_strided_group(int count, const float* const* A, const float* const* W, const float* const* bias, const float* const* mask,
                                     float* const* C, long sa_m, long sa_k, long sw_n, long sw_k, int ldmask, int ldc, int M, int N, int K, int act,
                                     float* splitk_ws, size_t splitk_ws_bytes, hipStream_t st) {
    if (M == 0 || N == 0 || count == 0) return SHASTA_OK;
    GemmGroup gg;
    bool va = true, vw = true, any_mask = false;
    for (int i = 0; i < GEMM_GROUP_MAX; ++i) {
        const int j = i < count ? i : 0;
        gg.A[i] = A[j];
        gg.W[i] = W[j];
        gg.bias[i] = bias ? bias[j] : nullptr;
        gg.mask[i] = mask ? mask[j] : nullptr;
        gg.C[i] = C[j];
        va = va && strided_vec_ok(sa_m, sa_k, A[j]);
        vw = vw && strided_vec_ok(sw_n, sw_k, W[j]);
        any_mask = any_mask || gg.mask[i] != nullptr;
    }
    gg.mtiles = cdiv(M, BM);
    const GemmStridedPlan p = plan_gemm_strided(M, N, K, act, any_mask, splitk_ws ? splitk_ws_bytes / count : 0);
    const bool split = p.slice_stride != 0;
    const GemmS g = gemm_strided_args(p, sa_m, sa_k, sw_n, sw_k, va, vw, ldmask, ldc, M, N, K, act);  // (pointers: group_member)
    GemmGroup gs = gg;  // split-K: the slices of member i at splitk_ws + i * nz * M * N
    for (int i = 0; split && i < GEMM_GROUP_MAX; ++i) {
        gs.C[i] = splitk_ws + (size_t)(i < count ? i : 0) * p.nz * M * N;
        gs.bias[i] = nullptr;
    }
    const dim3 grid(cdiv(N, BN), gg.mtiles * count, p.nz);
    if (act & 8) hipLaunchKernelGGL(gemm_strided_group_bf16_kernel, grid, dim3(256), 0, st, g, gs);
    else hipLaunchKernelGGL(gemm_strided_group_f32_kernel, grid, dim3(256), 0, st, g, gs);
    int rc = check_launch(split ? "gemm_strided_group(split-K)" : "gemm_strided_group");
    if (rc || !split) return rc;
    const long n = (long)M * N;
    hipLaunchKernelGGL(gemm_reduce_group_kernel, dim3((unsigned)((n + 15) / 16), count), dim3(256), 0, st, splitk_ws, p.slice_stride, p.nz, gg, n, N, ldc, act);
    return check_launch("gemm_reduce_group");
}

// the argument checks the two strided entries share; `entry`: the name the message starts with
static int check_gemm_strided_args(const char* entry, int ldc, int M, int N, int K, int act) {
    char msg[128];
    snprintf(msg, sizeof(msg), "%s: bad size", entry);
    SHASTA_REQUIRE(M >= 0 && N >= 0 && K >= 0 && ldc >= N, msg);
    snprintf(msg, sizeof(msg), "%s: bad activation (0 none, 1 relu, 2 abs, +4 accumulate into C, +8 bf16 operands)", entry);
    SHASTA_REQUIRE(act >= 0 && act <= 14 && (act & 3) != 3, msg);
    return SHASTA_OK;
}

}  // namespace shasta

extern "C" int shasta_gemm_strided_group_f32(int count, const float* const* A, const float* const* W, const float* const* bias,
                                             const float* const* relu_mask, float* const* C, long sa_m, long sa_k, long sw_n, long sw_k,
                                             int ldmask, int ldc, int M, int N, int K, int act, void* splitk_ws, size_t splitk_ws_bytes,
                                             shasta_stream_t stream) {
    using namespace shasta;
    SHASTA_REQUIRE(count >= 0 && count <= GEMM_GROUP_MAX, "gemm_strided_group: 0 to 8 members");
    SHASTA_REQUIRE(count == 0 || (A && W && C), "gemm_strided_group: null pointer");
    for (int i = 0; i < count; ++i) SHASTA_REQUIRE(A[i] && W[i] && C[i], "gemm_strided_group: null member pointer");
    if (int rc = check_gemm_strided_args("gemm_strided_group", ldc, M, N, K, act)) return rc;
    return launch_gemm_strided_group(count, A, W, bias, relu_mask, C, sa_m, sa_k, sw_n, sw_k, ldmask, ldc, M, N, K, act,
                                     static_cast<float*>(splitk_ws), splitk_ws_bytes, as_stream(stream));
}

extern "C" int shasta_gemm_strided_f32(const float* A, long sa_m, long sa_k, const float* W, long sw_n, long sw_k, const float* bias,
                                       const float* relu_mask, int ldmask, float* C, int ldc, int M, int N, int K, int act,
                                       void* splitk_ws, size_t splitk_ws_bytes, shasta_stream_t stream) {
    using namespace shasta;
    SHASTA_REQUIRE(A && W && C, "gemm_strided: null pointer");
    if (int rc = check_gemm_strided_args("gemm_strided", ldc, M, N, K, act)) return rc;
    return launch_gemm_strided(A, sa_m, sa_k, W, sw_n, sw_k, bias, relu_mask, ldmask, C, ldc, M, N, K, act,
                               static_cast<float*>(splitk_ws), splitk_ws_bytes, as_stream(stream));
}
