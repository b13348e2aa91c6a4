// K0 on the fp16 matrix path: shared_conv of the affinity network (det3d/models/tracker/shasta.py:42-47, applied :223-228)
//   Conv2d(Cin -> 64, 3x3, padding 1, bias) -> BatchNorm2d(64) in eval mode -> ReLU -> permute to NHWC
// with fp32 operands in HBM, fp32 accumulation and every fp32 product formed from THREE fp16 products (the two-piece form of the
// weight stream, anchor_split.hip):  a 2^e = a_h + a_l,  a_h = fp16(a 2^e),  a_l = fp16(a 2^e - a_h), both rounded to nearest;
// w x = w_l x_h + w_h x_l + w_h x_h (the dropped w_l x_l is below 2^-22 |w x|).  2^e is an exact power of two - one per OUTPUT CHANNEL for
// the weights (pack time), one per IMAGE for the activations (a max-reduction pass over the map, conv16_absmax_kernel) - that puts
// the largest magnitude into (2^13, 2^14]; the epilogue scales the sums back exactly.  v_mfma_f32_32x32x16_f16 forms 16x the
// products per cycle of v_mfma_f32_32x32x2_f32, so the 38.2 GFLOP of a frame pair have a 0.046 ms matrix floor instead of 0.24 ms.
//
// Implicit GEMM: M = pixels, N = 64 output channels (two 32-wide blocks), K = 9 taps x Cin, walked in chunks of 16 input channels
// (one k-step of 16 = one tap of one chunk; lane half h of an operand fragment holds channels 8h .. 8h+7).
// A workgroup (8 waves) owns 256 CONSECUTIVE pixels of the flattened image (254 workgroups per 180 x 180 map, no padding waste),
// wave w the 32 pixels 32w .. 32w+31 and both channel blocks (2 accumulators).  Per chunk:
//  * input tile: exactly the flat pixel range the 256 pixels touch (one image row + one pixel either side) is loaded along the
//    pixel axis (a lane = 1 pixel x 8 channels, three such items per lane), cut ONCE into its fp16 pieces on the VALU and written
//    to LDS as [piece][channel octet][padded pixel slot][8 fp16]: an operand fragment of a tap is one ds_read_b128 per lane at
//    (a per-lane base) + (a compile-time offset), lane-linear, i.e. conflict-free.  Slots are numbered as in an image whose rows
//    have one padding column either side: the padding slots are zeroed once and never written, so the x-boundary of the
//    convolution costs nothing in the loop (the y-boundary: rows outside the image are never written either).
//  * weights: pre-cut at pack time into the fragment order [chunk][tap][channel block][piece][lane][8 fp16] (36 KB per chunk) and
//    copied straight into LDS by LDS-DMA (global_load_lds_dwordx4), shared by the eight waves.
//  Both tiles are double buffered; one barrier per chunk.  The two waves of a SIMD (w, w+4) cut their share of the next input
//  tile at different points of the chunk, so that one of them always feeds the matrix pipe.
// Several class heads (the seven per-class models of tools/nusc_shasta, official_val.sh) run in ONE launch: blockIdx -> (tile, head)
// with the heads of a tile next to each other on one XCD, so the map is read from HBM once and 6 of 7 tile reads hit that L2.
#include "common.hpp"
#include "lds_dma.hpp"
#include "pieces.hpp"

#include <string.h>

#include <type_traits>

namespace shasta {

constexpr int C16_NW = 8;                      // waves per workgroup: two per SIMD
constexpr int C16_WBUF = 9 * 2 * 2 * 1024;     // [tap 9][channel block 2][piece 2] fragments of 1 KB
constexpr int C16_MAXH = 8;                    // class heads per launch
constexpr int C16_PARAMS = 320;                // floats behind the fragments: alpha[64], beta'[64], bias[64], 2^-e[64], then [256] = 1.0 for a RAW head
                                               // (train mode: conv + bias as is, no BatchNorm, no ReLU - shared_conv_train.hip takes it from there)

// The matrix kernel has three forms (256-pixel tiles, 512-pixel tiles, 512-pixel tiles of a pre-cut input: see each kernel).  They differ
// in the tile geometry below, in where the weight fragments live and in the schedule of one chunk; everything else - which tile a block
// works on, staging, operand addresses, the tap products and their order, the epilogue - is ONE piece of code, a template on the geometry.
template <int TILE_, int NSLOT_, int NIT_, int WBUFS_>
struct Conv16Geo {
    static constexpr int TILE = TILE_;                // pixels per workgroup
    static constexpr int PB = TILE_ / (32 * C16_NW);  // 32-pixel blocks per wave
    static constexpr int NSLOT = NSLOT_;              // padded pixel slots of one staged tile incl. the 8 trash slots at the end
    static constexpr int NIT = NIT_;                  // staged (64-pixel block, octet) items per lane and chunk: up to 8 NIT blocks over the waves
    static constexpr int PLANE = NSLOT_ * 16;         // bytes of one [slot][8 fp16] plane
    static constexpr int INBUF = 4 * PLANE;           // [piece 2][octet 2] planes
    static constexpr int IN0 = WBUFS_ * C16_WBUF;     // the two input buffers lie behind the weight region(s)
    static constexpr int LDS = IN0 + 2 * INBUF;       // one workgroup per CU
    static constexpr int wreg(int buf) { return buf % WBUFS_ * C16_WBUF; }  // the weight region read together with input buffer `buf`
};
using G256 = Conv16Geo<256, 640, 3, 2>;  // W = 180 needs 626 slots; weights double buffered: 155 648 bytes
using G512 = Conv16Geo<512, 912, 4, 1>;  // W = 187: 900 + 8 slots, 2 x 57 KB of input; one weight region: 153 600 bytes
using GPre = Conv16Geo<512, 896, 0, 1>;  // 14 LDS-DMA instructions of 1 KB per plane (W <= 185), nothing staged by the lanes: 151 552 bytes

// (the residuals f16_res_lo / f16_res_hi go through a compiler-generated conversion before anything else reads them: hazard rule of
// pieces.hpp)

// ---- pack: one workgroup per output channel --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv16_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ mean, const float* __restrict__ var, float eps, int Cin,
                                                          char* __restrict__ out, int raw) {
    __shared__ float red[4];
    const int n = blockIdx.x, tid = threadIdx.x, K = Cin * 9;
    const float* wn = w + (size_t)n * K;
    float m = 0.0f;
    for (int i = tid; i < K; i += 256) m = absmax_keep_nan(m, fabsf(wn[i]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = absmax_keep_nan(m, __shfl_xor(m, off, 64));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = absmax_keep_nan(absmax_keep_nan(red[0], red[1]), absmax_keep_nan(red[2], red[3]));
    const int e = range_exponent_bits(__float_as_uint(m));
    const int nchunk = Cin / 16, nb = n >> 5, nl = n & 31;
    for (int it = tid; it < nchunk * 18; it += 256) {
        const int c = it / 18, r = it - c * 18, tap = r >> 1, h = r & 1;
        u32x4 hi, lo;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            _Float16 h0, l0, h1, l1;
            cut2_f16(__builtin_ldexpf(wn[(16 * c + 8 * h + 2 * jj) * 9 + tap], e), h0, l0);
            cut2_f16(__builtin_ldexpf(wn[(16 * c + 8 * h + 2 * jj + 1) * 9 + tap], e), h1, l1);
            hi[jj] = pack_f16x2(h0, h1);
            lo[jj] = pack_f16x2(l0, l1);
        }
        char* f = out + (size_t)c * C16_WBUF + ((tap * 2 + nb) * 2) * 1024 + (h * 32 + nl) * 16;
        *reinterpret_cast<u32x4*>(f) = hi;
        *reinterpret_cast<u32x4*>(f + 1024) = lo;
    }
    if (tid == 0) {
        float* par = reinterpret_cast<float*>(out + (size_t)nchunk * C16_WBUF);
        const float alpha = raw ? 1.0f : (1.0f / sqrtf(var[n] + eps)) * gamma[n];
        par[n] = alpha;
        par[64 + n] = raw ? 0.0f : beta[n] - mean[n] * alpha;
        par[128 + n] = bias[n];
        par[192 + n] = __builtin_ldexpf(1.0f, -e);
        if (n == 0) par[256] = raw ? 1.0f : 0.0f;
    }
}

// ---- largest magnitude of every image: grid (slices, images); out[image] must be zero on entry ----------------------------------------
__global__ __launch_bounds__(256) void conv16_absmax_kernel(const float* __restrict__ xa, const float* __restrict__ xb, long per_image, int B,
                                                            unsigned* __restrict__ out) {
    __shared__ float red[4];
    const int z = blockIdx.y;
    const float* x = (z >= B ? xb + (size_t)(z - B) * per_image : xa + (size_t)z * per_image);
    const long n4 = per_image / 4, per = (n4 + gridDim.x - 1) / gridDim.x;
    const long beg = blockIdx.x * per, end = min(n4, beg + per);
    const f32x4* p = reinterpret_cast<const f32x4*>(x);
    float m = 0.0f;
    for (long i = beg + threadIdx.x; i < end; i += 256) {
        const f32x4 v = p[i];
        m = absmax_keep_nan(absmax_keep_nan(m, absmax_keep_nan(fabsf(v[0]), fabsf(v[1]))), absmax_keep_nan(fabsf(v[2]), fabsf(v[3])));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = absmax_keep_nan(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicMax(out + z, __float_as_uint(absmax_keep_nan(absmax_keep_nan(red[0], red[1]), absmax_keep_nan(red[2], red[3]))));
}

struct Conv16Args {
    const float* x[2];              // current / previous neck outputs (B, Cin, H, W)
    float* out[2][C16_MAXH];        // per head: (B, H, W, 64)
    const char* packed;             // heads x head_stride bytes
    size_t head_stride;
    const unsigned* xmax;           // [nmaps] bit patterns of the image maxima
    int B, Cin, H, W, heads, tiles_per_map, ntiles, tiles_per_xcd;
};

// ---- the pieces the three forms share --------------------------------------------------------------------------------------------
using B0 = std::integral_constant<int, 0>;
using B1 = std::integral_constant<int, 1>;
template <int N>
using IC = std::integral_constant<int, N>;

// Who a lane is: its wave (uniform), its number in the wave and its place in an MFMA operand or result (index li of 32, half h).  Filled
// once per kernel: the operand addresses and the epilogue use the same li and h.
struct Conv16Lane {
    int wv, lane, li, h;
};
__device__ __forceinline__ Conv16Lane conv16_lane() {
    const int tid = threadIdx.x, lane = tid & 63;
    return {__builtin_amdgcn_readfirstlane(tid >> 6), lane, lane & 31, lane >> 5};
}

// What a workgroup works on.
struct Conv16Tile {
    const float* xin;  // the image: channel 0 of its map
    float* out;        // this head's output for that image
    const char* wsrc;  // this head's packed fragments, its parameters behind them
    int z, W, WT, npix, nchunk;
    int eimg;          // the image's scale is 2^eimg
    int p0;            // first pixel of the tile
    int first;         // padded index (y * WT + x + 1) of pixel (y0 - 1, x0 - 1) = slot 0 of the staged tile
};
// block -> (tile, head): blocks 8 apart share an XCD; an XCD takes a contiguous range of tiles (neighbours share halo rows in
// its L2) and runs the heads of a tile back to back.  A block whose tile is not below a.ntiles has nothing to do: the kernels return on
// that themselves, before conv16_tile reads anything (a bool out of one function kept the flag alive and cost every later division by
// W its shared reciprocal).
__device__ __forceinline__ int conv16_block_tile(const Conv16Args& a) { return (blockIdx.x & 7) * a.tiles_per_xcd + (blockIdx.x >> 3) / a.heads; }
template <class G>
__device__ __forceinline__ Conv16Tile conv16_tile(const Conv16Args& a, int tt) {
    Conv16Tile t;
    const int head = (blockIdx.x >> 3) % a.heads;
    const int z = tt / a.tiles_per_map, tile = tt - z * a.tiles_per_map;
    const bool second = z >= a.B;
    const int b = second ? z - a.B : z;
    t.z = z;
    t.W = a.W;
    t.WT = a.W + 2;
    t.npix = a.H * a.W;
    t.nchunk = a.Cin / 16;
    t.xin = (second ? a.x[1] : a.x[0]) + (size_t)b * a.Cin * t.npix;
    t.out = (second ? a.out[1][head] : a.out[0][head]) + (size_t)b * t.npix * 64;
    t.wsrc = a.packed + (size_t)head * a.head_stride;
    t.eimg = range_exponent_bits(a.xmax[z]);
    t.p0 = tile * G::TILE;
    const int y0 = t.p0 / t.W, x0 = t.p0 - y0 * t.W;
    t.first = (y0 - 1) * t.WT + x0;
    return t;
}

// zero both input buffers once: padding slots and rows outside the image are never written afterwards
template <class G>
__device__ __forceinline__ void conv16_zero_inputs(char* lds, int tid) {
    const u32x4 zz = {0u, 0u, 0u, 0u};
    for (int i = tid; i < 2 * G::INBUF / 16; i += 64 * C16_NW) reinterpret_cast<u32x4*>(lds + G::IN0)[i] = zz;
}

// Staging roles of a lane: NIT (pixel, channel octet) items of every chunk.  The flat pixel range the tile touches is dealt in
// blocks of 64 consecutive pixels, first all blocks of octet 0, then those of octet 1; block 8 i + w goes to wave w as its item i:
// consecutive lanes = consecutive pixels, so the 4-byte loads of a channel row are whole 256-byte lines and the 16-byte LDS stores
// of a piece are lane-linear (a lane holding FOUR consecutive pixels would store 64 bytes apart: a 4-way bank conflict on every store)
template <class G>
struct Conv16Stage {
    int st_addr[G::NIT];      // LDS byte offset inside an input buffer (octet plane + slot); lanes without a pixel to stage point at one
                              // of the eight trash slots NSLOT - 8 .. - 1 of their octet plane, which no tap ever reads
    unsigned ld_off[G::NIT];  // byte offset of channel 0 of the octet inside a chunk; always a valid address
    bool item_live[G::NIT];   // wave-uniform: this wave's item holds pixels at all (its cut and stores are skipped otherwise)
    f32x2 scale2;             // the image's scale, twice
};
template <class G>
__device__ __forceinline__ void conv16_stage_roles(const Conv16Tile& t, const Conv16Lane& me, Conv16Stage<G>& s) {
    const int W = t.W, WT = t.WT, npix = t.npix;
    const int p_last = min(t.p0 + G::TILE, npix) - 1;
    const int qs = t.p0 - W - 1, qe = p_last + W + 1;  // first / last flat pixel a tap of this tile reads (may lie outside the image)
    const int nblk = (qe - qs + 64) >> 6;              // 64-pixel blocks per octet (the host guarantees 2 nblk <= 8 NIT)
#pragma unroll
    for (int it = 0; it < G::NIT; ++it) {
        const int blk = it * C16_NW + me.wv;
        const int oct = blk >= nblk ? 1 : 0;
        const int q = qs + 64 * (blk - oct * nblk) + me.lane;
        s.item_live[it] = blk < 2 * nblk;
        const bool ok = s.item_live[it] && q >= 0 && q < npix && q <= qe;
        const int yy = ok ? q / W : 0, xx = q - yy * W;
        const int sl = yy * WT + xx + 1 - t.first;
        s.st_addr[it] = (min(oct, 1) * G::PLANE) + ((ok && sl >= 0 && sl < G::NSLOT - 8) ? sl : G::NSLOT - 8 + (me.lane & 7)) * 16;  // (sl < 0: the pixel left of the halo when the tile starts a row)
        s.ld_off[it] = 4u * (unsigned)(oct * 8 * npix + (ok ? q : 0));
    }
    const float scale = __builtin_ldexpf(1.0f, t.eimg);
    s.scale2 = f32x2{scale, scale};
}

// The raw tile r[NIT][8] of a kernel travels in registers for a whole trip.  Its loads are inline asm: hipcc builds a 64-bit vector
// address per load otherwise (24 v_lshl_add_u64 per trip - vector instructions of a wave take issue slots from its SIMD partner's matrix
// instructions), and the waits can then be exact: the compiler knows nothing of these loads, every s_waitcnt vmcnt is ours.
template <class G>
__device__ __forceinline__ void conv16_load_chunk(const Conv16Tile& t, const Conv16Stage<G>& s, int ch, float (&r)[G::NIT][8]) {
    const char* xc = reinterpret_cast<const char*>(t.xin + (size_t)ch * 16 * t.npix);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const char* xj = uniform_ptr(xc + (size_t)j * t.npix * 4);
#pragma unroll
        for (int it = 0; it < G::NIT; ++it) {
            asm volatile("global_load_dword %0, %1, %2" : "=v"(r[it][j]) : "v"(s.ld_off[it]), "s"(xj) : "memory");
        }
    }
}
// wait until at most LEFT of this wave's youngest vector-memory operations are in flight, and tie r[] to the wait so that
// nothing reads a register before it has landed
template <class G, int LEFT>
__device__ __forceinline__ void conv16_wait_tile(float (&r)[G::NIT][8]) {
    asm volatile("s_waitcnt vmcnt(%8)"
                 : "+v"(r[0][0]), "+v"(r[0][1]), "+v"(r[0][2]), "+v"(r[0][3]), "+v"(r[0][4]), "+v"(r[0][5]), "+v"(r[0][6]), "+v"(r[0][7])
                 : "n"(LEFT));
#pragma unroll
    for (int it = 1; it < G::NIT; ++it)
        asm volatile("" : "+v"(r[it][0]), "+v"(r[it][1]), "+v"(r[it][2]), "+v"(r[it][3]), "+v"(r[it][4]), "+v"(r[it][5]), "+v"(r[it][6]), "+v"(r[it][7]));
}
// the raw tile, cut into its fp16 pieces, into input buffer BUF
template <class G, int BUF>
__device__ __forceinline__ void conv16_cut_store(char* lds, const Conv16Stage<G>& s, const float (&r)[G::NIT][8]) {
    constexpr int IB = G::IN0 + BUF * G::INBUF;
#pragma unroll
    for (int it = 0; it < G::NIT; ++it) {
        if (!s.item_live[it]) continue;  // wave-uniform
        u32x4 hi, lo;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {  // 2.5 vector instructions per value: packed scale, packed convert, two exact residuals, packed convert
            const f32x2 sv = f32x2{r[it][2 * jj], r[it][2 * jj + 1]} * s.scale2;
            const uint32_t hp = pack_f16x2((_Float16)sv[0], (_Float16)sv[1]);
            hi[jj] = hp;
            lo[jj] = pack_f16x2((_Float16)f16_res_lo(sv[0], hp), (_Float16)f16_res_hi(sv[1], hp));
        }
        *reinterpret_cast<u32x4*>(lds + IB + s.st_addr[it]) = hi;
        *reinterpret_cast<u32x4*>(lds + IB + 2 * G::PLANE + s.st_addr[it]) = lo;
    }
}

// LDS-DMA of weight fragments F0 .. of chunk ch into the weight region at LDS address wreg (the 36 fragments of a chunk lie in the
// packed buffer as in LDS): wave w copies fragments F0 + w, + 8, ..., CNT of them; lane_off = 16 lane
template <int F0, int CNT>
__device__ __forceinline__ void conv16_dma_frags(const char* wsrc, int ch, int wv, uint32_t wreg, uint32_t lane_off) {
    const char* src = wsrc + (size_t)ch * C16_WBUF + (F0 + wv) * 1024;
    const uint32_t dst0 = wreg + (uint32_t)((F0 + wv) * 1024);
#pragma unroll
    for (int j = 0; j < CNT; ++j) {
        const char* base = uniform_ptr(src + j * (C16_NW * 1024));
        const uint32_t dst = __builtin_amdgcn_readfirstlane(dst0 + (uint32_t)(j * (C16_NW * 1024)));
        lds_dma_x4(lane_off, base, dst);
    }
}

// operand addresses of a lane: pixel block pb of wave w = pixels 32 (PB w + pb) + (lane & 31) of the tile; a_row[pb][dy] = byte offset
// inside an input buffer of tap (dy, dx = 0), dx adds 16 bytes each
template <class G>
__device__ __forceinline__ void conv16_operand_rows(const Conv16Tile& t, const Conv16Lane& me, int (&a_row)[G::PB][3]) {
#pragma unroll
    for (int pb = 0; pb < G::PB; ++pb) {
        const int p = min(t.p0 + 32 * (G::PB * me.wv + pb) + me.li, t.npix - 1);
        const int py = p / t.W, px = p - py * t.W;
        const int sc = py * t.WT + px + 1 - t.first;  // slot of the pixel itself (>= WT + 1)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) a_row[pb][dy] = me.h * G::PLANE + (sc + (dy - 1) * t.WT - 1) * 16;
    }
}

// One tap of one chunk: its operand fragments, one ds_read_b128 each, and its products.  The order of the piece products - small to
// large, per accumulator - is what makes the three forms give the same bits.
template <int PB>
struct Conv16Frag {
    f16x8 ah[PB], al[PB], b0h, b0l, b1h, b1l;
};
template <class G, int BUF>
__device__ __forceinline__ void conv16_read_tap(const char* lds, const int (&a_row)[G::PB][3], int b_lane, int tap, Conv16Frag<G::PB>& f) {
    const char* ib = lds + G::IN0 + BUF * G::INBUF;
    const char* wb = lds + G::wreg(BUF) + b_lane;
    const int dy = tap / 3, dx = tap % 3;
#pragma unroll
    for (int pb = 0; pb < G::PB; ++pb) {
        f.ah[pb] = *reinterpret_cast<const f16x8*>(ib + a_row[pb][dy] + dx * 16);
        f.al[pb] = *reinterpret_cast<const f16x8*>(ib + a_row[pb][dy] + dx * 16 + 2 * G::PLANE);
    }
    f.b0h = *reinterpret_cast<const f16x8*>(wb + (tap * 4 + 0) * 1024);
    f.b0l = *reinterpret_cast<const f16x8*>(wb + (tap * 4 + 1) * 1024);
    f.b1h = *reinterpret_cast<const f16x8*>(wb + (tap * 4 + 2) * 1024);
    f.b1l = *reinterpret_cast<const f16x8*>(wb + (tap * 4 + 3) * 1024);
}
template <int PB>
__device__ __forceinline__ void conv16_mma_tap(const Conv16Frag<PB>& f, f32x16 (&acc)[PB][2]) {
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
        acc[pb][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[pb], f.b0h, acc[pb][0], 0, 0, 0);
        acc[pb][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[pb], f.b1h, acc[pb][1], 0, 0, 0);
    }
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
        acc[pb][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[pb], f.b0l, acc[pb][0], 0, 0, 0);
        acc[pb][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[pb], f.b1l, acc[pb][1], 0, 0, 0);
    }
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
        acc[pb][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[pb], f.b0h, acc[pb][0], 0, 0, 0);
        acc[pb][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[pb], f.b1h, acc[pb][1], 0, 0, 0);
    }
}

// every chunk in turn, chunk(ch, buffer parity): the parity is a compile-time constant (two trips per loop iteration, an odd tail)
template <class F>
__device__ __forceinline__ void conv16_all_chunks(int nchunk, F chunk) {
    int ch = 0;
#pragma unroll 1
    for (; ch + 1 < nchunk; ch += 2) {
        chunk(ch, B0{});
        chunk(ch + 1, B1{});
    }
    if (ch < nchunk) chunk(ch, B0{});
}

// epilogue: descale, bias, BatchNorm, ReLU (or the raw sums), NHWC store.  D[pixel][channel]: lane = channel (32 nb + li), pixel =
// (r & 3) + 8 (r >> 2) + 4 h of the block's 32
template <class G>
__device__ __forceinline__ void conv16_epilogue(const Conv16Tile& t, const Conv16Lane& me, const f32x16 (&acc)[G::PB][2]) {
    const float* par = reinterpret_cast<const float*>(t.wsrc + (size_t)t.nchunk * C16_WBUF);
    const float back = __builtin_ldexpf(1.0f, -t.eimg);
    const bool raw = par[256] != 0.0f;  // uniform
#pragma unroll
    for (int pb = 0; pb < G::PB; ++pb) {
        const int pblk = t.p0 + 32 * (G::PB * me.wv + pb);
        if (pblk >= t.npix) continue;  // wave-uniform
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int chn = 32 * nb + me.li;
            const float alpha = par[chn], beta2 = par[64 + chn], bias = par[128 + chn], un = par[192 + chn] * back;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int pp = pblk + (rr & 3) + 8 * (rr >> 2) + 4 * me.h;
                if (pp < t.npix) {
                    const float sv = acc[pb][nb][rr] * un;
                    const float v = (sv + bias) * alpha + beta2;
                    t.out[(size_t)pp * 64 + chn] = raw ? v : relu_nan(v);
                }
            }
        }
    }
}

// ---- 256-pixel tiles ---------------------------------------------------------------------------------------------------------------
// 8 waves (two per SIMD), each 32 pixels x 64 channels.  The 36 weight fragments of a chunk are dealt to the waves, wave w copies
// fragments w, w + 8, ...: waves 0-3 take five of them and cut the next tile early, their SIMD partners 4-7 four and cut late.
__global__ __launch_bounds__(512, 2) void shared_conv_f16_kernel(Conv16Args a) {
    using G = G256;
    constexpr int NLD = 8 * G::NIT;  // global loads of one staged chunk per lane
    static_assert(NLD + 5 <= 63, "vmcnt is 6 bits");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const Conv16Lane me = conv16_lane();
    const int wv = me.wv, lane = me.lane;
    const int tt = conv16_block_tile(a);
    if (tt >= a.ntiles) return;
    const Conv16Tile t = conv16_tile<G>(a, tt);
    conv16_zero_inputs<G>(lds, threadIdx.x);
    Conv16Stage<G> s;
    conv16_stage_roles<G>(t, me, s);
    float r[G::NIT][8];
    const uint32_t lds0 = (uint32_t)(size_t)((__attribute__((address_space(3))) char*)lds);
    const uint32_t dma_off = (uint32_t)(lane * 16);
    auto dma_weights = [&](int ch, int buf, auto ndma) __attribute__((always_inline)) {
        conv16_dma_frags<0, decltype(ndma)::value>(t.wsrc, ch, wv, lds0 + (uint32_t)G::wreg(buf), dma_off);
    };
    int a_row[G::PB][3];
    conv16_operand_rows<G>(t, me, a_row);
    const int b_lane = lane * 16;
    const f32x16 zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    f32x16 acc[G::PB][2] = {{zero16, zero16}};
    using Frag = Conv16Frag<G::PB>;

    const int nchunk = t.nchunk;
    const bool early = wv < 4;
    if (early) dma_weights(0, 0, IC<5>{});
    else dma_weights(0, 0, IC<4>{});
    conv16_load_chunk<G>(t, s, 0, r);
    __syncthreads();  // the zero fill is complete
    conv16_wait_tile<G, 0>(r);
    conv16_cut_store<G, 0>(lds, s, r);
    conv16_load_chunk<G>(t, s, min(1, nchunk - 1), r);
    // Everything has landed before the loop is entered, the second tile included: the compiler thinks an asm load's result is there
    // at once and may COPY it (it does, into the loop's registers, right behind this barrier) - a copy of a register whose load is
    // still in flight reads stale data.  Inside the loop the loads write the loop-carried registers themselves (checked in the ISA;
    // tests/test_hip_parity.py::test_shared_conv_vs_oracle fails loudly if a compiler ever changes that).
    conv16_wait_tile<G, 0>(r);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // One chunk.  On entry LDS holds chunk ch (tile + weights) and the registers r[] the raw tile of chunk ch + 1, on its way since the
    // middle of the previous trip: it is cut into the other buffer after CUT taps, and the loads of chunk ch + 2 follow at once, so a
    // load has a whole trip to land.  The last trips stage the last chunk again, into the buffer nobody reads any more: no branch in
    // the loop.  The fragments of tap t + 1 are read while tap t is multiplied.  The two waves of a SIMD (w, w + 4) cut at different
    // points of the trip, so that one of them always feeds the matrix pipe.  Waits: before the cut everything but this trip's LDS-DMA
    // (the loads are older), at the end everything but the NLD loads just issued (the LDS-DMA is older).
    auto chunk = [&](int ch, auto bufc, auto cut_after, auto ndma) __attribute__((always_inline)) {
        constexpr int CUT = decltype(cut_after)::value, CUR = decltype(bufc)::value, NDMA = decltype(ndma)::value;
        const int nxt = min(ch + 1, nchunk - 1), nx2 = min(ch + 2, nchunk - 1);
        dma_weights(nxt, CUR ^ 1, ndma);
        auto stage = [&]() __attribute__((always_inline)) {
            __builtin_amdgcn_sched_barrier(0);  // (the scheduler otherwise lifts the cut - and its wait for the loads - to the top of the trip)
            conv16_wait_tile<G, NDMA>(r);
            conv16_cut_store<G, CUR ^ 1>(lds, s, r);
            conv16_load_chunk<G>(t, s, nx2, r);
            __builtin_amdgcn_sched_barrier(0);
        };
        Frag fa, fb;
        conv16_read_tap<G, CUR>(lds, a_row, b_lane, 0, fa);
#pragma unroll
        for (int tap = 0; tap < 9; tap += 2) {
            if (tap + 1 < 9) conv16_read_tap<G, CUR>(lds, a_row, b_lane, tap + 1, fb);
            conv16_mma_tap(fa, acc);
            if (tap + 1 == CUT) stage();
            if (tap + 1 < 9) {
                if (tap + 2 < 9) conv16_read_tap<G, CUR>(lds, a_row, b_lane, tap + 2, fa);
                conv16_mma_tap(fb, acc);
                if (tap + 2 == CUT) stage();
            }
        }
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NLD) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    if (early) conv16_all_chunks(nchunk, [&](int ch, auto bufc) __attribute__((always_inline)) { chunk(ch, bufc, IC<2>{}, IC<5>{}); });
    else conv16_all_chunks(nchunk, [&](int ch, auto bufc) __attribute__((always_inline)) { chunk(ch, bufc, IC<6>{}, IC<4>{}); });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the staged-again last chunk: nothing may be in flight when the wave ends
    conv16_epilogue<G>(t, me, acc);
}

// ---- 512-pixel tiles (maps in bulk) -----------------------------------------------------------------------------------------------
// Per chunk the kernel above reads 432 KB of operand fragments out of LDS (3 375 cycles of its 128 B / clk) for 3 456 cycles of matrix
// work per SIMD: the two limits coincide and do not overlap perfectly - a chunk takes ~6 300 cycles.  Three quarters of those reads are
// the weight fragments, which every wave fetches for its single 32-pixel block.  Here a wave owns TWO pixel blocks (64 pixels x 64
// channels, four accumulators) and the workgroup of eight waves 512 consecutive pixels: a weight fragment feeds two MFMAs, 8 instead
// of 12 ds_read_b128 per 12 MFMAs, and the weights cross from L2 into LDS once per 512 pixels.  Two waves per SIMD as before.  LDS: the
// input tile grows to 2 x 57 KB (912 padded slots), so the weights of a chunk are no longer double-buffered whole: their 36 fragments
// sit in ONE 36 KB region in two halves - taps 0-4 and taps 5-8 - each refilled by LDS-DMA as soon as every wave has passed it (a
// barrier in the middle of the chunk, one at its end): half B of chunk c is requested at the top of chunk c and has the time of taps
// 0-4 to land, half A of chunk c + 1 is requested behind the middle barrier and has taps 5-8.
// Waits (every vector-memory operation of the loop is ours, see conv16_load_chunk): the waves that cut early (w < 4, the SIMD partners
// of the late ones) issue their 32 loads of chunk c + 2 between the two DMA batches of a trip - middle: everything but those loads,
// end: everything; the late waves issue them behind both - middle: everything, end: everything but the loads.
constexpr int W2_HALF = 20;  // fragments of taps 0-4

__global__ __launch_bounds__(512, 2) void shared_conv_f16w_kernel(Conv16Args a) {
    using G = G512;
    constexpr int NLD = 8 * G::NIT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const Conv16Lane me = conv16_lane();
    const int wv = me.wv, lane = me.lane;
    const int tt = conv16_block_tile(a);
    if (tt >= a.ntiles) return;
    const Conv16Tile t = conv16_tile<G>(a, tt);
    conv16_zero_inputs<G>(lds, threadIdx.x);
    Conv16Stage<G> s;
    conv16_stage_roles<G>(t, me, s);
    float r[G::NIT][8];
    const uint32_t lds0 = (uint32_t)(size_t)((__attribute__((address_space(3))) char*)lds);
    const uint32_t dma_off = (uint32_t)(lane * 16);
    auto dma_frags = [&](int ch, auto firstc, auto countc) __attribute__((always_inline)) {
        conv16_dma_frags<decltype(firstc)::value, decltype(countc)::value>(t.wsrc, ch, wv, lds0, dma_off);
    };
    int a_row[G::PB][3];
    conv16_operand_rows<G>(t, me, a_row);
    const int b_lane = lane * 16;
    const f32x16 zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    f32x16 acc[G::PB][2] = {{zero16, zero16}, {zero16, zero16}};
    using Frag = Conv16Frag<G::PB>;

    const int nchunk = t.nchunk;
    const bool early = wv < 4;  // three fragments of half A and the early cut; the SIMD partner w + 4: two and the late cut
    // prologue: all 36 fragments of chunk 0, tile 0 cut into buffer 0, the raw tile of chunk 1 in registers; everything has landed (see
    // the note at this point of the kernel above)
    if (early) dma_frags(0, IC<0>{}, IC<3>{});
    else dma_frags(0, IC<0>{}, IC<2>{});
    dma_frags(0, IC<W2_HALF>{}, IC<2>{});
    conv16_load_chunk<G>(t, s, 0, r);
    __syncthreads();  // the zero fill is complete
    conv16_wait_tile<G, 0>(r);
    conv16_cut_store<G, 0>(lds, s, r);
    conv16_load_chunk<G>(t, s, min(1, nchunk - 1), r);
    conv16_wait_tile<G, 0>(r);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // One chunk (EARLY / buffer parity compile-time).  On entry: LDS holds tile ch, ALL 36 weight fragments of chunk ch when ch == 0,
    // otherwise half A of chunk ch (half B still chunk ch - 1's, consumed by everybody: requested now); r[] = the raw tile of ch + 1.
    auto chunk = [&](int ch, auto bufc, auto earlyc) __attribute__((always_inline)) {
        constexpr int CUR = decltype(bufc)::value;
        constexpr bool EARLY = decltype(earlyc)::value;
        constexpr int CUT = EARLY ? 2 : 7;  // taps multiplied before this wave cuts the next tile
        const int nxt = min(ch + 1, nchunk - 1), nx2 = min(ch + 2, nchunk - 1);
        if (ch > 0) dma_frags(ch, IC<W2_HALF>{}, IC<2>{});  // half B of this chunk
        auto stage = [&]() __attribute__((always_inline)) {
            __builtin_amdgcn_sched_barrier(0);
            conv16_wait_tile<G, 2>(r);  // everything but the two fragments this wave requested last
            conv16_cut_store<G, CUR ^ 1>(lds, s, r);
            conv16_load_chunk<G>(t, s, nx2, r);
            __builtin_amdgcn_sched_barrier(0);
        };
        Frag fa, fb;
        conv16_read_tap<G, CUR>(lds, a_row, b_lane, 0, fa);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            Frag& cur = (tap & 1) ? fb : fa;
            Frag& nx = (tap & 1) ? fa : fb;
            if (tap + 1 < 9 && tap != 4) conv16_read_tap<G, CUR>(lds, a_row, b_lane, tap + 1, nx);  // (tap 5's weights: behind the middle barrier)
            conv16_mma_tap(cur, acc);
            if (tap + 1 == CUT) stage();
            if (tap == 4) {
                // middle: half B of this chunk has landed (this wave's share; the barrier: everybody's) and everybody is past half A,
                // which takes chunk ch + 1's fragments
                if (EARLY) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NLD) : "memory");
                else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                if (EARLY) dma_frags(nxt, IC<0>{}, IC<3>{});
                else dma_frags(nxt, IC<0>{}, IC<2>{});
                conv16_read_tap<G, CUR>(lds, a_row, b_lane, 5, nx);
            }
        }
        if (EARLY) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NLD) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    if (early) conv16_all_chunks(nchunk, [&](int ch, auto bufc) __attribute__((always_inline)) { chunk(ch, bufc, std::true_type{}); });
    else conv16_all_chunks(nchunk, [&](int ch, auto bufc) __attribute__((always_inline)) { chunk(ch, bufc, std::false_type{}); });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the staged-again last chunk and the last refill of half A: nothing in flight at the end
    conv16_epilogue<G>(t, me, acc);
}

// ---- the input cut once for all heads (maps in bulk, several class heads) ----------------------------------------------------------
// Ablation builds of the kernel above (removed after commit 96899a8; 8 frame pairs, one head): 0.89 ms with everything, 0.67 ms without its staging (loads,
// cut, LDS stores: the vector work that competes with the SIMD partner's matrix instructions), and the seven class heads of
// tools/nusc_shasta/eval.py:86-101 each cut the SAME input tile again.  Here a bandwidth-bound pre-pass (conv16_precut_kernel) cuts every
// map once into the fp16 piece image of ALL its tiles - [chunk][piece][octet][padded pixel slot][8 fp16], slots numbered as in the image
// with one zero column either side and one zero row above and below, i.e. exactly the numbering of the staged tiles - and a tile of any
// workgroup is a CONTIGUOUS window of that image: the matrix kernel (shared_conv_f16p_kernel) fetches it by LDS-DMA and holds nothing
// but DMA, ds_read and MFMA in its loop (no staging registers: 218 -> ~150 VGPRs).  Costs one write and one read of the map's worth of
// bytes extra (0.4 ms at 8 frame pairs): taken from three heads per launch on; 68 MB of workspace per map.
// slots of one plane of a map's piece image: the padded image and a zero tail as long as a tile window
static inline long conv16p_plane_slots(int H, int W) { return ((long)(H + 2) * (W + 2) + GPre::NSLOT + 63) / 64 * 64; }

// grid (ceil(plane slots / 256), 2 chunks-octets ..., maps): thread = (padded slot, octet) of one chunk
__global__ __launch_bounds__(256) void conv16_precut_kernel(const float* __restrict__ xa, const float* __restrict__ xb, int B, int Cin, int H, int W,
                                                            const unsigned* __restrict__ xmax, u32x4* __restrict__ img, long plane_slots) {
    const int z = blockIdx.z, co = blockIdx.y, ch = co >> 1, oct = co & 1;
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= plane_slots) return;
    const int WT = W + 2, npix = H * W;
    const long row = s / WT;
    const int xp = (int)(s - row * WT);
    const bool real = row >= 1 && row <= H && xp >= 1 && xp <= W;
    u32x4 hi = {0u, 0u, 0u, 0u}, lo = {0u, 0u, 0u, 0u};
    if (real) {
        const float* x = (z >= B ? xb + (size_t)(z - B) * Cin * npix : xa + (size_t)z * Cin * npix) + (size_t)(16 * ch + 8 * oct) * npix + (row - 1) * W + (xp - 1);
        const float scale = __builtin_ldexpf(1.0f, range_exponent_bits(xmax[z]));
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const float v0 = x[(size_t)(2 * jj) * npix] * scale, v1 = x[(size_t)(2 * jj + 1) * npix] * scale;
            const uint32_t hp = pack_f16x2((_Float16)v0, (_Float16)v1);
            hi[jj] = hp;
            lo[jj] = pack_f16x2((_Float16)f16_res_lo(v0, hp), (_Float16)f16_res_hi(v1, hp));
        }
    }
    u32x4* o = img + (((size_t)z * (Cin / 16) + ch) * 4 + oct) * plane_slots + s;
    o[0] = hi;
    o[2 * plane_slots] = lo;
}

struct Conv16pArgs {
    Conv16Args c;
    const char* img;   // [map][chunk][piece 2][octet 2][plane slots][16 B]
    long plane_slots;
};

__global__ __launch_bounds__(512, 2) void shared_conv_f16p_kernel(Conv16pArgs pa) {
    using G = GPre;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const Conv16Lane me = conv16_lane();
    const int wv = me.wv, lane = me.lane;
    const int tt = conv16_block_tile(pa.c);
    if (tt >= pa.c.ntiles) return;
    const Conv16Tile t = conv16_tile<G>(pa.c, tt);
    const int nchunk = t.nchunk;
    const long gidx0 = (long)t.first + t.WT;  // image slot of tile slot 0 = pixel (y0 - 1, x0 - 1): the image has one zero row above row 0
    const char* tsrc = pa.img + ((size_t)t.z * nchunk * 4 * pa.plane_slots + (size_t)gidx0) * 16;  // plane (chunk 0, piece 0, octet 0), slot gidx0
    const size_t plane_bytes = (size_t)pa.plane_slots * 16;

    const uint32_t lds0 = (uint32_t)(size_t)((__attribute__((address_space(3))) char*)lds);
    const uint32_t dma_off = (uint32_t)(lane * 16);
    auto dma_frags = [&](int ch, auto firstc, auto countc) __attribute__((always_inline)) {
        conv16_dma_frags<decltype(firstc)::value, decltype(countc)::value>(t.wsrc, ch, wv, lds0, dma_off);
    };
    // the tile of chunk ch into input buffer `buf`: 4 planes x 14 KB = 56 instructions of 1 KB, seven per wave (instruction 8 j + w)
    auto dma_tile = [&](int ch, int buf) __attribute__((always_inline)) {
        const uint32_t off = dma_off;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int i = 8 * j + wv, pl = i / 14, k = i - pl * 14;  // plane (piece * 2 + octet), KB within it
            const char* base = uniform_ptr(tsrc + ((size_t)ch * 4 + pl) * plane_bytes + (size_t)k * 1024);
            const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)(G::IN0 + buf * G::INBUF + pl * G::PLANE + k * 1024));
            lds_dma_x4(off, base, dst);
        }
    };
    int a_row[G::PB][3];
    conv16_operand_rows<G>(t, me, a_row);
    const int b_lane = lane * 16;
    const f32x16 zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    f32x16 acc[G::PB][2] = {{zero16, zero16}, {zero16, zero16}};
    using Frag = Conv16Frag<G::PB>;

    const bool three = wv < 4;  // three fragments of half A (the others two)
    // prologue: all 36 fragments and the tile of chunk 0
    if (three) dma_frags(0, IC<0>{}, IC<3>{});
    else dma_frags(0, IC<0>{}, IC<2>{});
    dma_frags(0, IC<W2_HALF>{}, IC<2>{});
    dma_tile(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // One chunk.  Top: half B of this chunk (2) and the next chunk's tile (7) are requested; middle: half B has landed (the 7 tile
    // requests are younger), barrier, half A of the next chunk is requested; end: everything has landed, barrier.
    auto chunk = [&](int ch, auto bufc, auto threec) __attribute__((always_inline)) {
        constexpr int CUR = decltype(bufc)::value;
        const int nxt = min(ch + 1, nchunk - 1);
        if (ch > 0) dma_frags(ch, IC<W2_HALF>{}, IC<2>{});
        dma_tile(nxt, CUR ^ 1);
        Frag fa, fb;
        conv16_read_tap<G, CUR>(lds, a_row, b_lane, 0, fa);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            Frag& cur = (tap & 1) ? fb : fa;
            Frag& nx = (tap & 1) ? fa : fb;
            if (tap + 1 < 9 && tap != 4) conv16_read_tap<G, CUR>(lds, a_row, b_lane, tap + 1, nx);
            conv16_mma_tap(cur, acc);
            if (tap == 4) {
                asm volatile("s_waitcnt vmcnt(7) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                dma_frags(nxt, IC<0>{}, threec);
                conv16_read_tap<G, CUR>(lds, a_row, b_lane, 5, nx);
            }
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    if (three) conv16_all_chunks(nchunk, [&](int ch, auto bufc) __attribute__((always_inline)) { chunk(ch, bufc, IC<3>{}); });
    else conv16_all_chunks(nchunk, [&](int ch, auto bufc) __attribute__((always_inline)) { chunk(ch, bufc, IC<2>{}); });
    conv16_epilogue<G>(t, me, acc);
}

// ---- which form serves a call -----------------------------------------------------------------------------------------------------
// slots one staged tile of `tile` pixels needs at this map width (see conv16_stage_roles: np + 2 WT + 2 + 2 x row wraps)
static int conv16_slots(int tile, int H, int W) {
    const int np = min(tile, H * W);
    const int wraps = (W - 1 + np - 1) / W;
    return np + 2 * (W + 2) + 2 + 2 * wraps;
}
// 64-pixel blocks, both octets, that the staging of such a tile deals over the waves
static int conv16_stage_blocks(int tile, int H, int W) { return 2 * ((min(tile, H * W) + 2 * W + 2 + 63) / 64); }
template <class G>
static bool conv16_staging_fits(int H, int W) {
    return conv16_slots(G::TILE, H, W) <= G::NSLOT - 8 && conv16_stage_blocks(G::TILE, H, W) <= C16_NW * G::NIT;
}
static size_t conv16p_image_bytes(int in_channels, int H, int W, int nmaps) {
    return (size_t)nmaps * (in_channels / 16) * 4 * (size_t)conv16p_plane_slots(H, W) * 16;
}

enum class Conv16Form { Tile256, Tile512, PreCut };
// The 512-pixel forms serve a launch when the map fits the staging of the 512-pixel kernel and there is enough work to fill the chip with
// their (half as many) tiles.  Of the two, the pre-cut form from three heads on, when the map fits its tile window (the smaller of the
// two, so the 512-pixel kernel can always stand in for it) and `room` bytes of workspace behind the image maxima hold the piece image.
static Conv16Form conv16_form(int in_channels, int H, int W, int nmaps, int heads, size_t room) {
    if (!conv16_staging_fits<G512>(H, W) || (long)cdiv(H * W, G512::TILE) * nmaps * heads < 512) return Conv16Form::Tile256;
    if (heads >= 3 && conv16_slots(GPre::TILE, H, W) <= GPre::NSLOT && room >= conv16p_image_bytes(in_channels, H, W, nmaps)) return Conv16Form::PreCut;
    return Conv16Form::Tile512;
}

}  // namespace shasta

using namespace shasta;

extern "C" int shasta_shared_conv_f16x2_supported(int in_channels, int H, int W) {
    if (in_channels <= 0 || in_channels % 16 || H <= 0 || W <= 0) return 0;
    if ((long)in_channels * H * W >= (1L << 31)) return 0;
    return conv16_staging_fits<G256>(H, W);  // (the 256-pixel form must serve the map: the larger forms are chosen per call)
}

extern "C" size_t shasta_shared_conv_f16x2_packed_bytes(int in_channels) {
    if (in_channels <= 0 || in_channels % 16) return 0;
    return (size_t)(in_channels / 16) * C16_WBUF + C16_PARAMS * sizeof(float);
}

extern "C" int shasta_shared_conv_pack_f16x2(const float* weight, const float* bias, const float* bn_weight, const float* bn_bias,
                                             const float* bn_mean, const float* bn_var, float bn_eps, int in_channels, void* packed,
                                             size_t packed_bytes, shasta_stream_t stream) {
    SHASTA_REQUIRE(weight && bias && bn_weight && bn_bias && bn_mean && bn_var && packed, "shared_conv_pack_f16x2: null pointer");
    SHASTA_REQUIRE(in_channels > 0 && in_channels % 16 == 0, "shared_conv_pack_f16x2: in_channels must be a multiple of 16");
    SHASTA_REQUIRE((uintptr_t)packed % 16 == 0, "shared_conv_pack_f16x2: packed buffer must be 16-byte aligned");
    if (packed_bytes < shasta_shared_conv_f16x2_packed_bytes(in_channels)) {
        set_error_msg("shared_conv_pack_f16x2: packed buffer too small");
        return SHASTA_E_WORKSPACE;
    }
    hipLaunchKernelGGL(conv16_pack_kernel, dim3(64), dim3(256), 0, as_stream(stream), weight, bias, bn_weight, bn_bias, bn_mean, bn_var,
                       bn_eps, in_channels, static_cast<char*>(packed), 0);
    return check_launch("shared_conv_pack_f16x2");
}

extern "C" int shasta_shared_conv_pack_raw_f16x2(const float* weight, const float* bias, int in_channels, void* packed, size_t packed_bytes,
                                                 shasta_stream_t stream) {
    SHASTA_REQUIRE(weight && bias && packed, "shared_conv_pack_raw_f16x2: null pointer");
    SHASTA_REQUIRE(in_channels > 0 && in_channels % 16 == 0, "shared_conv_pack_raw_f16x2: in_channels must be a multiple of 16");
    SHASTA_REQUIRE((uintptr_t)packed % 16 == 0, "shared_conv_pack_raw_f16x2: packed buffer must be 16-byte aligned");
    if (packed_bytes < shasta_shared_conv_f16x2_packed_bytes(in_channels)) {
        set_error_msg("shared_conv_pack_raw_f16x2: packed buffer too small");
        return SHASTA_E_WORKSPACE;
    }
    hipLaunchKernelGGL(conv16_pack_kernel, dim3(64), dim3(256), 0, as_stream(stream), weight, bias, nullptr, nullptr, nullptr, nullptr, 0.0f,
                       in_channels, static_cast<char*>(packed), 1);
    return check_launch("shared_conv_pack_raw_f16x2");
}

extern "C" size_t shasta_shared_conv_multi_workspace_bytes(int B) { return B <= 0 ? 0 : align_up((size_t)2 * B * sizeof(unsigned), 256); }

extern "C" size_t shasta_shared_conv_multi_workspace_bytes_for(int B, int in_channels, int H, int W, int heads, int two_maps) {
    if (B <= 0 || in_channels <= 0 || in_channels % 16 || H <= 0 || W <= 0) return 0;
    const int nmaps = two_maps ? 2 * B : B;
    size_t n = shasta_shared_conv_multi_workspace_bytes(B);
    if (conv16_form(in_channels, H, W, nmaps, heads, SIZE_MAX) == Conv16Form::PreCut) n += conv16p_image_bytes(in_channels, H, W, nmaps);
    return n;
}

static int conv_multi(const float* x, const float* x_prev, int B, int in_channels, int H, int W, const void* packed, size_t head_stride_bytes,
                      int heads, float* const* h_out, float* const* h_out_prev, void* workspace, size_t workspace_bytes, float x_bound,
                      shasta_stream_t stream);

extern "C" int shasta_shared_conv_multi_f32(const float* x, const float* x_prev, int B, int in_channels, int H, int W, const void* packed,
                                            size_t head_stride_bytes, int heads, float* const* h_out, float* const* h_out_prev,
                                            void* workspace, size_t workspace_bytes, shasta_stream_t stream) {
    return conv_multi(x, x_prev, B, in_channels, H, W, packed, head_stride_bytes, heads, h_out, h_out_prev, workspace, workspace_bytes, 0.0f, stream);
}

extern "C" int shasta_shared_conv_multi_bounded_f32(const float* x, const float* x_prev, int B, int in_channels, int H, int W, const void* packed,
                                                    size_t head_stride_bytes, int heads, float* const* h_out, float* const* h_out_prev,
                                                    void* workspace, size_t workspace_bytes, float x_absmax_bound, shasta_stream_t stream) {
    SHASTA_REQUIRE(x_absmax_bound > 0.0f && x_absmax_bound < INFINITY, "shared_conv_multi_bounded: the bound must be positive and finite");
    return conv_multi(x, x_prev, B, in_channels, H, W, packed, head_stride_bytes, heads, h_out, h_out_prev, workspace, workspace_bytes,
                      x_absmax_bound, stream);
}

static int conv_multi(const float* x, const float* x_prev, int B, int in_channels, int H, int W, const void* packed, size_t head_stride_bytes,
                      int heads, float* const* h_out, float* const* h_out_prev, void* workspace, size_t workspace_bytes, float x_bound,
                      shasta_stream_t stream) {
    SHASTA_REQUIRE(x && packed && h_out, "shared_conv_multi: null pointer");
    SHASTA_REQUIRE((x_prev == nullptr) == (h_out_prev == nullptr), "shared_conv_multi: x_prev and h_out_prev go together");
    SHASTA_REQUIRE(heads >= 1 && heads <= C16_MAXH, "shared_conv_multi: 1 to 8 heads per call");
    SHASTA_REQUIRE(B >= 0 && H > 0 && W > 0, "shared_conv_multi: bad size");
    SHASTA_REQUIRE(shasta_shared_conv_f16x2_supported(in_channels, H, W),
                   "shared_conv_multi: shape not served by the fp16 kernel (in_channels % 16, map width; see shasta_shared_conv_f16x2_supported)");
    SHASTA_REQUIRE((uintptr_t)packed % 16 == 0 && head_stride_bytes % 16 == 0, "shared_conv_multi: packed buffer / head stride must be 16-byte aligned");
    SHASTA_REQUIRE(head_stride_bytes >= shasta_shared_conv_f16x2_packed_bytes(in_channels) || heads == 1, "shared_conv_multi: head stride too small");
    if (B == 0) return SHASTA_OK;
    SHASTA_REQUIRE(workspace, "shared_conv_multi: null workspace");
    if (workspace_bytes < shasta_shared_conv_multi_workspace_bytes(B)) {
        set_error_msg("shared_conv_multi: workspace too small");
        return SHASTA_E_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    const int nmaps = x_prev ? 2 * B : B;
    const long per_image = (long)in_channels * H * W;
    unsigned* xmax = static_cast<unsigned*>(workspace);
    int rc = SHASTA_OK;
    if (x_bound > 0.0f) {
        // the caller vouches for max |x| <= x_bound (the producer of the maps knows it): every image is cut under the bound's scale and
        // the maps are not read a second time.  The bound need not be tight (a piece pair keeps 22 bits of every element within 2^-17
        // of it); an element beyond 4 x the bound overflows fp16 and comes out as a NaN / Inf, never as a wrong finite number
        unsigned bits;
        memcpy(&bits, &x_bound, sizeof(bits));
        if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(xmax), (int)bits, (size_t)nmaps, st) != hipSuccess) return SHASTA_E_LAUNCH;
    } else {
        if (hipMemsetAsync(xmax, 0, (size_t)nmaps * sizeof(unsigned), st) != hipSuccess) return SHASTA_E_LAUNCH;
        int slices = 1;
        while (slices < 1024 && slices * nmaps < 2048 && per_image / (slices * 2) >= 16384) slices *= 2;
        hipLaunchKernelGGL(conv16_absmax_kernel, dim3(slices, nmaps), dim3(256), 0, st, x, x_prev, per_image, B, xmax);
        if ((rc = check_launch("shared_conv_multi (image maxima)")) != SHASTA_OK) return rc;
    }

    Conv16Args a;
    a.x[0] = x;
    a.x[1] = x_prev;
    for (int i = 0; i < C16_MAXH; ++i) {
        a.out[0][i] = i < heads ? h_out[i] : nullptr;
        a.out[1][i] = (i < heads && h_out_prev) ? h_out_prev[i] : nullptr;
        if (i < heads) SHASTA_REQUIRE(a.out[0][i] && (!h_out_prev || a.out[1][i]), "shared_conv_multi: null output pointer");
    }
    a.packed = static_cast<const char*>(packed);
    a.head_stride = head_stride_bytes;
    a.xmax = xmax;
    a.B = B;
    a.Cin = in_channels;
    a.H = H;
    a.W = W;
    a.heads = heads;
    // several heads over many maps and a workspace that holds the piece image: the input is cut once for all of them.  A device that
    // grants a form less LDS than it asks for gets the next smaller one.
    const size_t maxima_bytes = shasta_shared_conv_multi_workspace_bytes(B);
    Conv16Form form = conv16_form(in_channels, H, W, nmaps, heads, workspace_bytes - maxima_bytes);
    if (form == Conv16Form::PreCut &&
        hipFuncSetAttribute((const void*)shared_conv_f16p_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, GPre::LDS) != hipSuccess) {
        (void)hipGetLastError();
        form = Conv16Form::Tile512;
    }
    if (form == Conv16Form::Tile512 &&
        hipFuncSetAttribute((const void*)shared_conv_f16w_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, G512::LDS) != hipSuccess) {
        (void)hipGetLastError();
        form = Conv16Form::Tile256;
    }
    a.tiles_per_map = cdiv(H * W, form == Conv16Form::Tile256 ? G256::TILE : G512::TILE);
    a.ntiles = a.tiles_per_map * nmaps;
    a.tiles_per_xcd = cdiv(a.ntiles, 8);
    const dim3 grid(8 * a.tiles_per_xcd * heads), block(64 * C16_NW);
    if (form == Conv16Form::PreCut) {
        Conv16pArgs pa;
        pa.c = a;
        pa.plane_slots = conv16p_plane_slots(H, W);
        char* img = static_cast<char*>(workspace) + maxima_bytes;
        pa.img = img;
        hipLaunchKernelGGL(conv16_precut_kernel, dim3((unsigned)cdiv((int)pa.plane_slots, 256), 2 * (in_channels / 16), nmaps), dim3(256), 0, st, x, x_prev, B,
                           in_channels, H, W, xmax, reinterpret_cast<u32x4*>(img), pa.plane_slots);
        if ((rc = check_launch("shared_conv_multi (piece image)")) != SHASTA_OK) return rc;
        hipLaunchKernelGGL(shared_conv_f16p_kernel, grid, block, GPre::LDS, st, pa);
        return check_launch("shared_conv_f16p");
    }
    if (form == Conv16Form::Tile512) {
        hipLaunchKernelGGL(shared_conv_f16w_kernel, grid, block, G512::LDS, st, a);
        return check_launch("shared_conv_f16w");
    }
    (void)hipFuncSetAttribute((const void*)shared_conv_f16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, G256::LDS);
    hipLaunchKernelGGL(shared_conv_f16_kernel, grid, block, G256::LDS, st, a);
    return check_launch("shared_conv_f16");
}
