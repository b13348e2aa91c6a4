// The sparse 3-D backbone SpMiddleResNetFHD (det3d/models/backbones/scn.py:98-211) layer by layer, eval mode, strict fp32: the index
// kernels (output coordinates of a strided level, neighbour tables), one gather-form convolution kernel for every layer, and the densify.
// Coordinates are (batch, z, y, x) int32 rows; a level's grid is (D, H, W).  No float atomics anywhere; the integer atomics only set bits.
//
// INDEX OF A LEVEL (caller-owned workspace, SpIndex in sp_index.hpp): a bitmap of the B x D x H x W grid (bit `lin` = cell
// ((b D + z) H + y) W + x is active), an exclusive prefix count of the set bits per 32-bit word (two-level: per word inside a block of
// 1024 words, and per block), and perm[rank] = row of the cell that is the rank-th active one in linear order.  A lookup is two loads, a
// popcount and perm[]; it is exact (no hash collisions, no probing) and independent of the order the bits were set in.
//   * rows given by the caller (the voxeliser's order, level conv1): set bits -> scan -> perm[rank(row)] = row.
//   * a strided level: every input row sets the bits of the <= ceil(k / s)^3 output sites it reaches -> scan -> the coordinates are
//     EMITTED in rank order, i.e. sorted by linear index, perm = identity, the count left in a device word.  The row order of a level
//     therefore depends on the set of active cells only, never on timing.
// Every coordinate that becomes an address is range-checked; a row outside the grid sets no bit (inactive) and a neighbour index outside
// [0, n_in) is treated as absent by the convolution.
//
// CONVOLUTION (spconv_layer_kernel<CK, NB>): output stationary.  A workgroup (256 threads, 4 waves) owns 128 output rows x all Cout.  It
// loads the tile's (128 x K) slice of the neighbour table into LDS once, then walks the taps in (kz, ky, kx) row-major order; a tap no row
// of the tile has is skipped (a workgroup-uniform flag: adding zeros changes no bit).  Per tap and per chunk of CK input channels the
// gathered rows (transposed: s_a[channel][row], row stride 129 floats -> conflict-free MFMA operand reads) and the tap's CK x Cout weight
// slice are staged through LDS; wave w multiplies rows 32 w .. 32 w + 31 on v_mfma_f32_32x32x2_f32 (A = gathered rows, B = weights:
// a D register of a lane = one output row, lanes = 32 consecutive channels -> 128-byte stores), Cout / 32 accumulators of 16 registers.
// Cout = 16: v_mfma_f32_16x16x4_f32, two accumulators of 4 registers (rows 0-15, 16-31 of the wave).  Per output a fixed-order fp32
// chain: taps, then channels.  Epilogue as neck.hip's: y = acc * alpha + beta' (bias and BatchNorm folded at pack time), + residual row,
// ReLU.
//
//   CK (input channels per chunk): 8 for Cin <= 8, 16 for Cin = 16, 32 for Cin = 32, 64, 128.  Compiler's resource report, the same for
//   every CK; no scratch in any kernel:
//   Cout   accumulators   VGPR + AGPR   LDS bytes (CK = 32)   waves / SIMD
//   16     2 x 4          32 +  8       32 492                5
//   32     1 x 16         30 + 16       34 540                4
//   64     2 x 16         60 + 32       38 636                4
//   128    4 x 16         92 + 64       46 828                3
//
// Packed layer: [tap][Cin rounded up to 8][Cout] weights (from the spconv 2.x layout (Cout, kD, kH, kW, Cin); channels >= Cin are
// zeros), then alpha[Cout], beta'[Cout]: alpha = gamma / sqrt(var + eps), beta' = beta + (bias - mean) * alpha.
#include "common.hpp"
#include "sp_index.hpp"  // SpIndex, sp_rank, sp_scan, the emit kernel (shared with dynvox.hip)

namespace shasta {

constexpr int SC_TM = 128;       // output rows per workgroup
constexpr int SC_AS = SC_TM + 1; // row stride of the transposed gather tile
constexpr int SC_KMAX = 27;

struct SpGeom {
    int k[3], s[3], p[3];
};

static bool sp_geom_ok(const SpGeom& g) {
    for (int a = 0; a < 3; ++a)
        if ((g.k[a] != 1 && g.k[a] != 3) || (g.s[a] != 1 && g.s[a] != 2) || (g.p[a] != 0 && g.p[a] != 1)) return false;
    return true;
}
static int sp_out_dim(int I, int k, int s, int p) { return (I + 2 * p - k) / s + 1; }
static bool sp_grid_ok(int B, int D, int H, int W) {
    return B >= 1 && D >= 1 && H >= 1 && W >= 1 && (double)B * D * H * W < 2147483648.0;
}
static int sp_cin_pad(int Cin) { return Cin <= 8 ? 8 : Cin; }
static bool sp_channels_ok(int Cin, int Cout) {
    const bool in_ok = (Cin >= 1 && Cin <= 8) || Cin == 16 || Cin == 32 || Cin == 64 || Cin == 128;
    return in_ok && (Cout == 16 || Cout == 32 || Cout == 64 || Cout == 128);
}
static bool sp_taps_ok(int K) { return K == 1 || K == 3 || K == 9 || K == 27; }

__global__ void sp_mark_rows_kernel(const int* __restrict__ coords, int n, int B, int D, int H, int W, uint32_t* __restrict__ bits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = coords[4 * (size_t)i], z = coords[4 * (size_t)i + 1], y = coords[4 * (size_t)i + 2], x = coords[4 * (size_t)i + 3];
    if ((unsigned)b >= (unsigned)B || (unsigned)z >= (unsigned)D || (unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return;
    const int lin = ((b * D + z) * H + y) * W + x;
    atomicOr(&bits[lin >> 5], 1u << (lin & 31));
}

// one thread per (input row, tap): the output site o with o * s - p + t = i, where there is one
__global__ void sp_mark_out_kernel(const int* __restrict__ coords, int n, int B, int D, int H, int W, SpGeom g, int Do, int Ho, int Wo,
                                   uint32_t* __restrict__ bits) {
    const int K = g.k[0] * g.k[1] * g.k[2];
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)n * K) return;
    const int i = (int)(id / K), tap = (int)(id - (long)i * K);
    const int b = coords[4 * (size_t)i], z = coords[4 * (size_t)i + 1], y = coords[4 * (size_t)i + 2], x = coords[4 * (size_t)i + 3];
    if ((unsigned)b >= (unsigned)B || (unsigned)z >= (unsigned)D || (unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return;
    const int tz = tap / (g.k[1] * g.k[2]), ty = (tap / g.k[2]) % g.k[1], tx = tap % g.k[2];
    const int nz = z + g.p[0] - tz, ny = y + g.p[1] - ty, nx = x + g.p[2] - tx;
    if (nz < 0 || ny < 0 || nx < 0 || nz % g.s[0] || ny % g.s[1] || nx % g.s[2]) return;
    const int oz = nz / g.s[0], oy = ny / g.s[1], ox = nx / g.s[2];
    if (oz >= Do || oy >= Ho || ox >= Wo) return;
    const int lin = ((b * Do + oz) * Ho + oy) * Wo + ox;
    atomicOr(&bits[lin >> 5], 1u << (lin & 31));
}

__global__ void sp_perm_rows_kernel(const int* __restrict__ coords, int n, int B, int D, int H, int W, const uint32_t* __restrict__ bits,
                                    const uint32_t* __restrict__ pre, const uint32_t* __restrict__ sums, int* __restrict__ perm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = coords[4 * (size_t)i], z = coords[4 * (size_t)i + 1], y = coords[4 * (size_t)i + 2], x = coords[4 * (size_t)i + 3];
    if ((unsigned)b >= (unsigned)B || (unsigned)z >= (unsigned)D || (unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return;
    const int r = sp_rank(bits, pre, sums, ((b * D + z) * H + y) * W + x);
    if (r >= 0 && r < n) perm[r] = i;  // (unique coordinates: every rank below the count is written once)
}

// one thread per (output row, tap): the input row at o * s - p + t, or -1
__global__ void sp_neighbors_kernel(const int* __restrict__ out_coords, int n_out, int B, int D, int H, int W, SpGeom g,
                                    const uint32_t* __restrict__ bits, const uint32_t* __restrict__ pre, const uint32_t* __restrict__ sums,
                                    const int* __restrict__ perm, int n_in, int* __restrict__ nbr) {
    const int K = g.k[0] * g.k[1] * g.k[2];
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)n_out * K) return;
    const int o = (int)(id / K), tap = (int)(id - (long)o * K);
    const int b = out_coords[4 * (size_t)o];
    const long oz = out_coords[4 * (size_t)o + 1], oy = out_coords[4 * (size_t)o + 2], ox = out_coords[4 * (size_t)o + 3];
    const int tz = tap / (g.k[1] * g.k[2]), ty = (tap / g.k[2]) % g.k[1], tx = tap % g.k[2];
    const long z = oz * g.s[0] - g.p[0] + tz, y = oy * g.s[1] - g.p[1] + ty, x = ox * g.s[2] - g.p[2] + tx;
    int j = -1;
    if ((unsigned)b < (unsigned)B && z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W) {
        const int r = sp_rank(bits, pre, sums, ((b * D + (int)z) * H + (int)y) * W + (int)x);
        if (r >= 0 && r < n_in) {
            j = perm[r];
            if ((unsigned)j >= (unsigned)n_in) j = -1;
        }
    }
    nbr[id] = j;
}

__global__ void sp_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ gamma,
                               const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var, float eps,
                               int Cin, int cin_pad, int Cout, int K, long total, float* __restrict__ out) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    for (long e = tid; e < total; e += nth) {
        const int co = (int)(e % Cout);
        const int c = (int)((e / Cout) % cin_pad);
        const int tap = (int)(e / Cout / cin_pad);
        out[e] = c < Cin ? w[((size_t)co * K + tap) * Cin + c] : 0.0f;  // (Cout, kD, kH, kW, Cin)
    }
    for (long n = tid; n < Cout; n += nth) {
        const float alpha = (1.0f / sqrtf(var[n] + eps)) * gamma[n];
        const float b0 = bias ? bias[n] : 0.0f;
        out[total + n] = alpha;
        out[total + Cout + n] = beta[n] + (b0 - mean[n]) * alpha;
    }
}

// x: (n_in, cin_real) rows; cin_pad = the packed layer's input channels (a multiple of CK); NB = Cout / 32, 0 for Cout = 16
template <int CK, int NB>
__global__ __launch_bounds__(256) void spconv_layer_kernel(const float* __restrict__ x, int cin_real, int cin_pad, int n_in,
                                                           const int* __restrict__ nbr, int K, int n_out, const float* __restrict__ packed,
                                                           const float* residual, int relu, float* out) {
    constexpr int COUT = NB ? 32 * NB : 16;
    constexpr int NACC = NB ? NB : 2;
    __shared__ float s_a[CK * SC_AS];
    __shared__ __attribute__((aligned(16))) float s_w[CK * COUT];
    __shared__ int s_nbr[SC_KMAX * SC_TM];
    __shared__ int s_flag[SC_KMAX];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t row0 = (size_t)blockIdx.x * SC_TM;

    if (tid < SC_KMAX) s_flag[tid] = 0;
    __syncthreads();
    for (int e = tid; e < K * SC_TM; e += 256) {  // the tile's slice of the (n_out, K) table is contiguous
        const int r = e / K, tap = e - r * K;
        int j = -1;
        if (row0 + r < (size_t)n_out) j = nbr[row0 * K + e];
        if ((unsigned)j >= (unsigned)n_in) j = -1;
        s_nbr[tap * SC_TM + r] = j;
        if (j >= 0) s_flag[tap] = 1;
    }
    __syncthreads();

    typedef float accv __attribute__((ext_vector_type(NB ? 16 : 4)));
    accv acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int r = 0; r < (NB ? 16 : 4); ++r) acc[a][r] = 0.0f;

    const int nchunk = cin_pad / CK;
#pragma unroll 1
    for (int tap = 0; tap < K; ++tap) {
        if (!s_flag[tap]) continue;  // workgroup-uniform
        const int* tn = s_nbr + tap * SC_TM;
#pragma unroll 1
        for (int ch = 0; ch < nchunk; ++ch) {
            __syncthreads();  // the previous chunk's operand reads are done
            if constexpr (CK == 8) {  // rows of cin_real <= 8 floats, any alignment
                for (int e = tid; e < SC_TM * 8; e += 256) {
                    const int r = e >> 3, c = e & 7;
                    const int j = tn[r];
                    float v = 0.0f;
                    if (j >= 0 && c < cin_real) v = x[(size_t)j * cin_real + c];
                    s_a[c * SC_AS + r] = v;
                }
            } else {
                constexpr int QPR = CK / 4;
                for (int e = tid; e < SC_TM * QPR; e += 256) {
                    const int r = e / QPR, q = e - r * QPR;
                    const int j = tn[r];
                    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (j >= 0) v = *reinterpret_cast<const f32x4*>(x + (size_t)j * cin_real + ch * CK + 4 * q);
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) s_a[(4 * q + jj) * SC_AS + r] = v[jj];
                }
            }
            const f32x4* wsrc = reinterpret_cast<const f32x4*>(packed + ((size_t)tap * cin_pad + (size_t)ch * CK) * COUT);
            for (int e = tid; e < CK * COUT / 4; e += 256) reinterpret_cast<f32x4*>(s_w)[e] = wsrc[e];
            __syncthreads();
            if constexpr (NB > 0) {
                const int i = lane & 31, h = lane >> 5;
                const float* pa = s_a + h * SC_AS + 32 * wv + i;
                const float* pb = s_w + h * COUT + i;
#pragma unroll
                for (int kk = 0; kk < CK / 2; ++kk) {
                    const float a = pa[2 * kk * SC_AS];
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
                        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, pb[2 * kk * COUT + 32 * nb], acc[nb], 0, 0, 0);
                }
            } else {
                const int i = lane & 15, q = lane >> 4;
                const float* pa = s_a + q * SC_AS + 32 * wv + i;
                const float* pb = s_w + q * COUT + i;
#pragma unroll
                for (int kk = 0; kk < CK / 4; ++kk) {
                    const float b = pb[4 * kk * COUT];
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[4 * kk * SC_AS], b, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[4 * kk * SC_AS + 16], b, acc[1], 0, 0, 0);
                }
            }
        }
    }

    const float* par = packed + (size_t)K * cin_pad * COUT;
    if constexpr (NB > 0) {  // D: channel = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 h
        const int i = lane & 31, h = lane >> 5;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int chn = 32 * nb + i;
            const float alpha = par[chn], beta = par[COUT + chn];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const size_t row = row0 + 32 * wv + mfma32_row(r, h);
                if (row < (size_t)n_out) {
                    float v = acc[nb][r] * alpha + beta;
                    if (residual) v += residual[row * COUT + chn];
                    out[row * COUT + chn] = relu ? relu_nan(v) : v;
                }
            }
        }
    } else {  // D: channel = lane & 15, row = 4 (lane >> 4) + r
        const int i = lane & 15, q = lane >> 4;
        const float alpha = par[i], beta = par[COUT + i];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t row = row0 + 32 * wv + 16 * t + 4 * q + r;
                if (row < (size_t)n_out) {
                    float v = acc[t][r] * alpha + beta;
                    if (residual) v += residual[row * COUT + i];
                    out[row * COUT + i] = relu ? relu_nan(v) : v;
                }
            }
    }
}

// out: (B, C, D, H, W) = (B, C D, H, W), zero-filled by the caller's memset before this kernel
__global__ void sp_dense_kernel(const float* __restrict__ feat, const int* __restrict__ coords, int n, int B, int C, int D, int H, int W,
                                float* __restrict__ out) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)n * C) return;
    const int i = (int)(id / C), c = (int)(id - (long)i * C);
    const int b = coords[4 * (size_t)i], z = coords[4 * (size_t)i + 1], y = coords[4 * (size_t)i + 2], x = coords[4 * (size_t)i + 3];
    if ((unsigned)b >= (unsigned)B || (unsigned)z >= (unsigned)D || (unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return;
    out[((((size_t)b * C + c) * D + z) * H + y) * W + x] = feat[id];
}

static int sp_zero(void* p, size_t bytes, hipStream_t st, const char* what) {
    const hipError_t e = hipMemsetAsync(p, 0, bytes, st);
    if (e != hipSuccess) {
        set_error(what, e);
        return SHASTA_E_LAUNCH;
    }
    return SHASTA_OK;
}

template <int CK>
static void sp_launch_layer(int Cout, dim3 grid, hipStream_t st, const float* x, int Cin, int cin_pad, int n_in, const int* nbr, int K,
                            int n_out, const float* pk, const float* residual, int relu, float* out) {
#define SHASTA_SP_LAUNCH(NB) \
    hipLaunchKernelGGL((spconv_layer_kernel<CK, NB>), grid, dim3(256), 0, st, x, Cin, cin_pad, n_in, nbr, K, n_out, pk, residual, relu, out)
    if (Cout == 16) SHASTA_SP_LAUNCH(0);
    else if (Cout == 32) SHASTA_SP_LAUNCH(1);
    else if (Cout == 64) SHASTA_SP_LAUNCH(2);
    else SHASTA_SP_LAUNCH(4);
#undef SHASTA_SP_LAUNCH
}

}  // namespace shasta

using namespace shasta;

#define SP_GEOM(g) const SpGeom g = {{kd, kh, kw}, {sd, sh, sw}, {pd, ph, pw}}

extern "C" int shasta_spconv_supported(int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw) {
    SP_GEOM(g);
    return sp_channels_ok(Cin, Cout) && sp_geom_ok(g) ? 1 : 0;
}

extern "C" size_t shasta_spconv_index_workspace_bytes(int B, int D, int H, int W, int rows) {
    if (!sp_grid_ok(B, D, H, W) || rows < 0) return 0;
    return SpIndex(nullptr, B, D, H, W, rows).bytes;
}

extern "C" int shasta_spconv_index_rows(const int* coords, int n, int B, int D, int H, int W, void* index_workspace, size_t workspace_bytes,
                                        shasta_stream_t stream) {
    SHASTA_REQUIRE(index_workspace && (coords || n == 0) && n >= 0, "spconv_index_rows: null pointer or negative row count");
    if (!sp_grid_ok(B, D, H, W)) {
        set_error_msg("spconv_index_rows: the grid needs B, D, H, W >= 1 and fewer than 2^31 cells");
        return SHASTA_E_UNSUPPORTED;
    }
    if ((uintptr_t)index_workspace % 16) {
        set_error_msg("spconv_index_rows: workspace must be 16-byte aligned");
        return SHASTA_E_ALIGN;
    }
    const SpIndex ix(index_workspace, B, D, H, W, n);
    if (workspace_bytes < ix.bytes) {
        set_error_msg("spconv_index_rows: workspace too small");
        return SHASTA_E_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    if (sp_zero(ix.bits, ix.words * 4, st, "spconv_index_rows") != SHASTA_OK) return SHASTA_E_LAUNCH;
    if (n > 0) hipLaunchKernelGGL(sp_mark_rows_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, coords, n, B, D, H, W, ix.bits);
    const int rc = sp_scan(ix, nullptr, st);
    if (rc != SHASTA_OK) return rc;
    if (n > 0)
        hipLaunchKernelGGL(sp_perm_rows_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, coords, n, B, D, H, W, ix.bits, ix.pre, ix.sums, ix.perm);
    return check_launch("spconv_index_rows");
}

extern "C" int shasta_spconv_out_coords(const int* coords, int n_in, int B, int D, int H, int W, int kd, int kh, int kw, int sd, int sh,
                                        int sw, int pd, int ph, int pw, int* out_coords, int out_capacity, int* n_out,
                                        void* index_workspace, size_t workspace_bytes, shasta_stream_t stream) {
    SHASTA_REQUIRE(index_workspace && n_out && (coords || n_in == 0) && n_in >= 0 && (out_coords || out_capacity == 0) && out_capacity >= 0,
                   "spconv_out_coords: null pointer or negative count");
    SP_GEOM(g);
    if (!sp_geom_ok(g) || !sp_grid_ok(B, D, H, W)) {
        set_error_msg("spconv_out_coords: kernel 1 or 3, stride 1 or 2, padding 0 or 1 per axis; a grid of fewer than 2^31 cells");
        return SHASTA_E_UNSUPPORTED;
    }
    const int Do = sp_out_dim(D, kd, sd, pd), Ho = sp_out_dim(H, kh, sh, ph), Wo = sp_out_dim(W, kw, sw, pw);
    if (D + 2 * pd < kd || H + 2 * ph < kh || W + 2 * pw < kw || !sp_grid_ok(B, Do, Ho, Wo) || (double)n_in * 27 >= 2147483648.0 * 256) {
        set_error_msg("spconv_out_coords: the output grid is empty or too large");
        return SHASTA_E_UNSUPPORTED;
    }
    if ((uintptr_t)index_workspace % 16) {
        set_error_msg("spconv_out_coords: workspace must be 16-byte aligned");
        return SHASTA_E_ALIGN;
    }
    const SpIndex ix(index_workspace, B, Do, Ho, Wo, out_capacity);
    if (workspace_bytes < ix.bytes) {
        set_error_msg("spconv_out_coords: workspace too small");
        return SHASTA_E_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    if (sp_zero(ix.bits, ix.words * 4, st, "spconv_out_coords") != SHASTA_OK) return SHASTA_E_LAUNCH;
    const long work = (long)n_in * kd * kh * kw;
    if (work > 0)
        hipLaunchKernelGGL(sp_mark_out_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, coords, n_in, B, D, H, W, g, Do, Ho, Wo,
                           ix.bits);
    const int rc = sp_scan(ix, n_out, st);
    if (rc != SHASTA_OK) return rc;
    if (out_capacity > 0)
        hipLaunchKernelGGL(sp_index_emit_kernel, dim3((unsigned)((ix.words + 255) / 256)), dim3(256), 0, st, ix.bits, ix.pre, ix.sums, ix.words,
                           Do, Ho, Wo, out_capacity, out_coords, ix.perm);
    return check_launch("spconv_out_coords");
}

extern "C" int shasta_spconv_neighbors(const int* out_coords, int n_out, int B, int D, int H, int W, int kd, int kh, int kw, int sd, int sh,
                                       int sw, int pd, int ph, int pw, const void* index_workspace, size_t workspace_bytes, int n_in,
                                       int* neighbors, shasta_stream_t stream) {
    SHASTA_REQUIRE(index_workspace && n_out >= 0 && n_in >= 0 && ((out_coords && neighbors) || n_out == 0),
                   "spconv_neighbors: null pointer or negative count");
    SP_GEOM(g);
    if (!sp_geom_ok(g) || !sp_grid_ok(B, D, H, W) || (double)n_out * 27 >= 2147483648.0) {
        set_error_msg("spconv_neighbors: kernel 1 or 3, stride 1 or 2, padding 0 or 1 per axis; a grid of fewer than 2^31 cells");
        return SHASTA_E_UNSUPPORTED;
    }
    if ((uintptr_t)index_workspace % 16) {
        set_error_msg("spconv_neighbors: workspace must be 16-byte aligned");
        return SHASTA_E_ALIGN;
    }
    const SpIndex ix(const_cast<void*>(index_workspace), B, D, H, W, n_in);
    if (workspace_bytes < ix.bytes) {
        set_error_msg("spconv_neighbors: index workspace too small for this grid and row count");
        return SHASTA_E_WORKSPACE;
    }
    const long work = (long)n_out * kd * kh * kw;
    if (work == 0) return SHASTA_OK;
    hipLaunchKernelGGL(sp_neighbors_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, as_stream(stream), out_coords, n_out, B, D, H,
                       W, g, ix.bits, ix.pre, ix.sums, ix.perm, n_in, neighbors);
    return check_launch("spconv_neighbors");
}

extern "C" size_t shasta_spconv_layer_packed_bytes(int Cin, int Cout, int K) {
    if (!sp_channels_ok(Cin, Cout) || !sp_taps_ok(K)) return 0;
    return ((size_t)K * sp_cin_pad(Cin) * Cout + 2 * (size_t)Cout) * sizeof(float);
}

extern "C" int shasta_spconv_layer_pack_f32(const float* weight, const float* bias, const float* bn_weight, const float* bn_bias,
                                            const float* bn_mean, const float* bn_var, float bn_eps, int Cin, int Cout, int K, void* packed,
                                            size_t packed_bytes, shasta_stream_t stream) {
    SHASTA_REQUIRE(weight && bn_weight && bn_bias && bn_mean && bn_var && packed, "spconv_layer_pack: null pointer");
    if (!sp_channels_ok(Cin, Cout) || !sp_taps_ok(K)) {
        set_error_msg("spconv_layer_pack: Cin <= 8, 16, 32, 64 or 128; Cout 16, 32, 64 or 128; 1, 3, 9 or 27 taps");
        return SHASTA_E_UNSUPPORTED;
    }
    if ((uintptr_t)packed % 16) {
        set_error_msg("spconv_layer_pack: packed buffer must be 16-byte aligned");
        return SHASTA_E_ALIGN;
    }
    if (packed_bytes < shasta_spconv_layer_packed_bytes(Cin, Cout, K)) {
        set_error_msg("spconv_layer_pack: packed buffer too small");
        return SHASTA_E_WORKSPACE;
    }
    const int cin_pad = sp_cin_pad(Cin);
    const long total = (long)K * cin_pad * Cout;
    hipLaunchKernelGGL(sp_pack_kernel, dim3(128), dim3(256), 0, as_stream(stream), weight, bias, bn_weight, bn_bias, bn_mean, bn_var, bn_eps,
                       Cin, cin_pad, Cout, K, total, static_cast<float*>(packed));
    return check_launch("spconv_layer_pack");
}

extern "C" int shasta_spconv_layer_f32(const float* x, int n_in, int Cin, const int* neighbors, int n_out, int K, const void* packed,
                                       size_t packed_bytes, int Cout, const float* residual, int relu, float* out, shasta_stream_t stream) {
    SHASTA_REQUIRE(packed && n_in >= 0 && n_out >= 0 && (x || n_in == 0) && ((neighbors && out) || n_out == 0),
                   "spconv_layer: null pointer or negative row count");
    if (!sp_channels_ok(Cin, Cout) || !sp_taps_ok(K)) {
        set_error_msg("spconv_layer: unsupported layer (Cin <= 8, 16, 32, 64 or 128; Cout 16, 32, 64 or 128; 1, 3, 9 or 27 taps)");
        return SHASTA_E_UNSUPPORTED;
    }
    if ((double)n_out * 27 >= 2147483648.0) {
        set_error_msg("spconv_layer: too many output rows for one call");
        return SHASTA_E_UNSUPPORTED;
    }
    if ((uintptr_t)packed % 16 || (Cin > 8 && (uintptr_t)x % 16)) {
        set_error_msg("spconv_layer: packed buffer and feature rows must be 16-byte aligned");
        return SHASTA_E_ALIGN;
    }
    if (packed_bytes < shasta_spconv_layer_packed_bytes(Cin, Cout, K)) {
        set_error_msg("spconv_layer: packed buffer too small");
        return SHASTA_E_WORKSPACE;
    }
    if (n_out == 0) return SHASTA_OK;
    SHASTA_REQUIRE(out != x, "spconv_layer: out must not alias x (rows are gathered by other workgroups)");
    const dim3 grid(cdiv(n_out, SC_TM));
    const float* pk = static_cast<const float*>(packed);
    hipStream_t st = as_stream(stream);
    const int cin_pad = sp_cin_pad(Cin);
    if (Cin <= 8) sp_launch_layer<8>(Cout, grid, st, x, Cin, cin_pad, n_in, neighbors, K, n_out, pk, residual, relu, out);
    else if (Cin == 16) sp_launch_layer<16>(Cout, grid, st, x, Cin, cin_pad, n_in, neighbors, K, n_out, pk, residual, relu, out);
    else sp_launch_layer<32>(Cout, grid, st, x, Cin, cin_pad, n_in, neighbors, K, n_out, pk, residual, relu, out);
    return check_launch("spconv_layer");
}

extern "C" int shasta_spconv_dense_f32(const float* features, const int* coords, int n, int B, int C, int D, int H, int W, float* out,
                                       shasta_stream_t stream) {
    SHASTA_REQUIRE(out && n >= 0 && ((features && coords) || n == 0), "spconv_dense: null pointer or negative row count");
    SHASTA_REQUIRE(C >= 1, "spconv_dense: bad channel count");
    if (!sp_grid_ok(B, D, H, W)) {
        set_error_msg("spconv_dense: the grid needs B, D, H, W >= 1 and fewer than 2^31 cells");
        return SHASTA_E_UNSUPPORTED;
    }
    hipStream_t st = as_stream(stream);
    if (sp_zero(out, (size_t)B * C * D * H * W * sizeof(float), st, "spconv_dense") != SHASTA_OK) return SHASTA_E_LAUNCH;
    const long work = (long)n * C;
    if (work > 0)
        hipLaunchKernelGGL(sp_dense_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, features, coords, n, B, C, D, H, W, out);
    return check_launch("spconv_dense");
}
