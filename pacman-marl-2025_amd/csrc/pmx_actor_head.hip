// pmx_actor_head.hip -- the first layer of MAPPOAgent.actor_head, Linear(32 H W -> 512) (pacman_mappo_resnet.py:117-119), on the
// matrix cores: the product between the fused tower (pmx_actor_forward, features [B][H W][32] bf16, cell-major) and the head tail
// (pmx_actor_tail_forward, h [B][512] bf16).  K = 32 H W is the contraction index of the forward product, k = cell * 32 + ch in the
// features' order; nn.Linear stores its weight with column ch * HW + cell (nn.Flatten's order).
//
//   pack      w [512][K] f32 (parameter order) -> Wp [512][Kp] bf16, cell-major, Kp = K rounded up to the 64-deep k-step, zero filled,
//             and (a second small kernel) WpT [K][512] bf16, its transpose, the operand of the input-gradient product
//   forward   h = feat . Wp^T + b          M = B, N = 512, K: split over K into float32 slabs, summed in slab order with the bias
//   dfeat     dfeat = dh . Wp              M = B, N = K, contraction 512, bf16 out
//   dW, db    dW = dh^T . feat             both operands batch-major: fragments through transposing LDS reads; the batch is split
//             over blocks into float32 slabs; the row-sum pass adds them in slab order and stores in the parameter's (ch, cell) order
//
// All three products share one structure: a 128 x 128 output tile per 256-thread workgroup (2 x 2 waves, 4 x 4 accumulators of
// v_mfma_f32_16x16x32_bf16 each), 64-deep steps, both operand tiles staged with 16-byte global_load_lds into ONE LDS array whose
// image is lane-linear (the XOR swizzle is applied to the SOURCE address), two barriers per step, bijective XCD remap of the block
// id.  No float atomics anywhere: every partial sum has its own slab and the sums run in a fixed order.
#pragma clang fp contract(fast)
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "../../include/pmx.h"
#include "pmx_common.h"

extern "C" int pmx_actor_supported(int32_t H, int32_t W);

namespace {

constexpr int HID = 512;              // output features of the layer
constexpr int TILE = 128;             // output tile side
constexpr int BK = 64;                // contraction depth of one step
constexpr int TILE_BYTES = TILE * BK * 2;          // 16 KiB per operand tile, either orientation
constexpr int FWD_BLOCKS = 256;       // forward: split K until about one block per CU
constexpr int FWD_MAX_SPLIT = 64;
constexpr int WG_BLOCKS = 512;        // weight gradient: split the batch until about two blocks per CU
constexpr int DB_ROWS = 64;           // partial rows of the bias gradient

__device__ __forceinline__ unsigned short bf_one(float a) { return (unsigned short)(bf_pack(a, 0.f) & 0xFFFFu); }

// 16 bytes from global memory (per-lane address) to LDS (wave-uniform base + 16 * lane)
__device__ __forceinline__ void glds16(const void *g, void *lds_wave_base)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g, (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, 0);
}
// every staged byte has landed in LDS (vmcnt counts the LDS-DMA loads), then the workgroup barrier
__device__ __forceinline__ void staged_barrier()
{
    __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0), expcnt and lgkmcnt left at their maxima
    __syncthreads();
}

// blocks b, b + 8, b + 16, .. share an XCD and its L2: hand each XCD a contiguous range of work ids (bijective for any grid size)
__device__ __forceinline__ int xcd_remap(int orig, int nwg)
{
    const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

// ---------------------------------------------------------------------------------------------------------------
// C[M][N] = A[M][.] . Bm[N][.]^T, both operands contraction-major (row reads).  LDS image of a tile: [128 rows][8 chunks of 16 B],
// chunk c of row r at slot c ^ (r & 7).  Rows past the operand's last are read from its last row (their results are never stored);
// A's chunks past a_chunks (the half step a K that is no multiple of 64 leaves) are read 4 chunks earlier in the same row and meet
// the zero padding of Bm.
//   MODE 0: float32 slab  out[(split * M + m) * N + n]     MODE 1: bfloat16 out[m * N + n] (+ bias[n] in float32 before the rounding)
// ---------------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void pmx_head_gemm_nt_kernel(const char *__restrict__ A, const char *__restrict__ Bm, const float *__restrict__ bias,
                                                              void *__restrict__ out, int M, int N, int lda_bytes, int ldb_bytes, int a_chunks,
                                                              int ksteps, int steps_per_split, int tiles_m, int tiles_n)
{
    __shared__ __attribute__((aligned(16))) char smem[2 * TILE_BYTES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wr = wv >> 1, wc = wv & 1, g = lane >> 4, fr = lane & 15;
    int id = xcd_remap(blockIdx.x, gridDim.x);
    const int tn = id % tiles_n;
    id /= tiles_n;
    const int tm = id % tiles_m, split = id / tiles_m;
    const int m0 = tm * TILE, n0 = tn * TILE;
    const int k_lo = split * steps_per_split, k_hi = min(ksteps, k_lo + steps_per_split);

    // staging: instruction i of wave wv fills chunk positions (4 i + wv) * 64 .. + 63 of each tile; this lane's position p -> row p >> 3,
    // slot p & 7, which holds the source chunk (p & 7) ^ (row & 7)
    const char *a_row[4], *b_row[4];
    int src_chunk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = (4 * i + wv) * 64 + lane, r = p >> 3;
        src_chunk[i] = (p & 7) ^ (r & 7);
        a_row[i] = A + (size_t)min(m0 + r, M - 1) * lda_bytes;
        b_row[i] = Bm + (size_t)min(n0 + r, N - 1) * ldb_bytes;
    }
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ks = k_lo; ks < k_hi; ++ks) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int ca = ks * 8 + src_chunk[i];
            ca = ca < a_chunks ? ca : ca - 4;
            glds16(a_row[i] + (size_t)ca * 16, smem + (4 * i + wv) * 1024);
            glds16(b_row[i] + (size_t)(ks * 8 + src_chunk[i]) * 16, smem + TILE_BYTES + (4 * i + wv) * 1024);
        }
        staged_barrier();
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 fa[4], fb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ra = wr * 64 + i * 16 + fr, rb = wc * 64 + i * 16 + fr;
                fa[i] = *reinterpret_cast<const bf16x8 *>(smem + ra * 128 + (((kk * 4 + g) ^ (ra & 7)) << 4));
                fb[i] = *reinterpret_cast<const bf16x8 *>(smem + TILE_BYTES + rb * 128 + (((kk * 4 + g) ^ (rb & 7)) << 4));
            }
            // the weight-side fragment as the A operand: D[n][m], so a lane owns 4 consecutive n of one m and stores them as one piece
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + wr * 64 + i * 16 + fr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wc * 64 + j * 16 + 4 * g;
            if (m < M && n < N) {
                const f32x4 v = acc[i][j];
                if (MODE == 0) {
                    *reinterpret_cast<float4 *>(reinterpret_cast<float *>(out) + ((size_t)split * M + m) * N + n) = float4{v[0], v[1], v[2], v[3]};
                } else {
                    float4 bv = float4{0.f, 0.f, 0.f, 0.f};
                    if (bias) bv = float4{bias[n], bias[n + 1], bias[n + 2], bias[n + 3]};      // (a parameter slice: 4-byte aligned only)
                    *reinterpret_cast<uint2 *>(reinterpret_cast<unsigned short *>(out) + (size_t)m * N + n) =
                        uint2{bf_pack(v[0] + bv.x, v[1] + bv.y), bf_pack(v[2] + bv.z, v[3] + bv.w)};
                }
            }
        }
    }
}

// h[b][n] = bf16(bias[n] + slab 0 + slab 1 + ..), the slabs added in their order; a thread owns 4 consecutive n
__global__ __launch_bounds__(256) void pmx_head_fwd_sum_kernel(const float *__restrict__ slab, const float *__restrict__ bias, unsigned short *__restrict__ h,
                                                              int64_t quads, int64_t slab_floats, int splits)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const float *bq = bias + 4 * (q & (HID / 4 - 1));                   // (a parameter slice: 4-byte aligned only)
    const float4 bv = float4{bq[0], bq[1], bq[2], bq[3]};
    float4 s = *reinterpret_cast<const float4 *>(slab + 4 * q);
    for (int k = 1; k < splits; ++k) {
        const float4 t = *reinterpret_cast<const float4 *>(slab + (size_t)k * slab_floats + 4 * q);
        s.x += t.x, s.y += t.y, s.z += t.z, s.w += t.w;
    }
    *reinterpret_cast<uint2 *>(h + 4 * q) = uint2{bf_pack(s.x + bv.x, s.y + bv.y), bf_pack(s.z + bv.z, s.w + bv.w)};
}

// ---------------------------------------------------------------------------------------------------------------
// Weight gradient: slab[c][n][k] = sum over the chunk's samples b of dh[b][n] feat[b][k].  Both tiles are [64 samples][128 columns]
// bf16 (256-byte rows); chunk ch of row r sits at slot ch ^ f(r), f(r) = ((r & 3) << 2) | ((r >> 2) & 3), the image whose transposing
// reads are conflict-free.  Samples past B are staged from sample B - 1 and then zeroed in LDS; feature columns past K are staged
// from the row's last chunk and never stored.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int tr_swz(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }

// the 16x16x32 operand fragment of columns col0 .. col0 + 15 over the 32 staged samples s0 .. s0 + 31 (contraction over samples)
__device__ __forceinline__ bf16x8 tr_frag(const char *tile, int s0, int col0, int lane)
{
    const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const int r_lo = s0 + 8 * g + q, r_hi = r_lo + 4, ch = (col0 >> 3) + (p >> 1);
    const char *a_lo = tile + r_lo * 256 + ((ch ^ tr_swz(r_lo)) << 4) + 8 * (p & 1);
    const char *a_hi = tile + r_hi * 256 + ((ch ^ tr_swz(r_hi)) << 4) + 8 * (p & 1);
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bf16x4 __attribute__((address_space(3))) *)(a_lo));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bf16x4 __attribute__((address_space(3))) *)(a_hi));
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

__global__ __launch_bounds__(256) void pmx_head_wgrad_kernel(const char *__restrict__ dh, const char *__restrict__ feat, float *__restrict__ slab,
                                                            int B, int K, int steps_per_chunk, int tiles_k)
{
    __shared__ __attribute__((aligned(16))) char smem[2 * TILE_BYTES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wr = wv >> 1, wc = wv & 1, g = lane >> 4, fr = lane & 15;
    int id = xcd_remap(blockIdx.x, gridDim.x);
    const int tk = id % tiles_k;
    id /= tiles_k;
    const int tn = id & 3, chunk = id >> 2;
    const int n0 = tn * TILE, k0 = tk * TILE;
    const int nsteps = (B + BK - 1) / BK;
    const int s_lo = chunk * steps_per_chunk, s_hi = min(nsteps, s_lo + steps_per_chunk);
    const int k_chunks = K >> 3;

    // staging position p = (4 i + wv) * 64 + lane -> row p >> 4, slot p & 15 holding source chunk (p & 15) ^ f(row)
    int st_row[4];
    size_t d_off[4], f_off[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = (4 * i + wv) * 64 + lane, r = p >> 4, c = (p & 15) ^ tr_swz(r);
        st_row[i] = r;
        d_off[i] = (size_t)((n0 >> 3) + c) * 16;
        f_off[i] = (size_t)min((k0 >> 3) + c, k_chunks - 1) * 16;
    }
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int s = s_lo; s < s_hi; ++s) {
        const int b0 = s * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const size_t b = (size_t)min(b0 + st_row[i], B - 1);
            glds16(dh + b * (HID * 2) + d_off[i], smem + (4 * i + wv) * 1024);
            glds16(feat + b * ((size_t)K * 2) + f_off[i], smem + TILE_BYTES + (4 * i + wv) * 1024);
        }
        staged_barrier();
        if (b0 + BK > B) {                                               // the ragged last step: samples past B contribute nothing
            const int first = B - b0;                                    // 1 .. 63
            for (int e = first * 16 + threadIdx.x; e < BK * 16; e += 256) {
                *reinterpret_cast<uint4 *>(smem + e * 16) = uint4{0u, 0u, 0u, 0u};
                *reinterpret_cast<uint4 *>(smem + TILE_BYTES + e * 16) = uint4{0u, 0u, 0u, 0u};
            }
            __syncthreads();
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 fd[4], ff[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ff[i] = tr_frag(smem + TILE_BYTES, kk * 32, wr * 64 + i * 16, lane);
                fd[i] = tr_frag(smem, kk * 32, wc * 64 + i * 16, lane);
            }
            // the feature-side fragment as the A operand: D[k][n], a lane owns 4 consecutive k of one n
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ff[i], fd[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    float *my = slab + (size_t)chunk * HID * K;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + wr * 64 + i * 16 + 4 * g;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wc * 64 + j * 16 + fr;
            if (k < K) {
                const f32x4 v = acc[i][j];
                *reinterpret_cast<float4 *>(my + (size_t)n * K + k) = float4{v[0], v[1], v[2], v[3]};
            }
        }
    }
}

// partial[p][n] = sum of dh[b][n] over the p-th slice of the batch; a thread owns two adjacent columns
__global__ __launch_bounds__(256) void pmx_head_db_partial_kernel(const uint32_t *__restrict__ dh, float *__restrict__ partial, int B, int rows_per_block)
{
    const int b_lo = blockIdx.x * rows_per_block, b_hi = min(B, b_lo + rows_per_block);
    float s0 = 0.f, s1 = 0.f;
    for (int b = b_lo; b < b_hi; ++b) {
        const uint32_t u = dh[(size_t)b * (HID / 2) + threadIdx.x];
        s0 += __uint_as_float(u << 16), s1 += __uint_as_float(u & 0xFFFF0000u);
    }
    partial[blockIdx.x * HID + 2 * threadIdx.x] = s0;
    partial[blockIdx.x * HID + 2 * threadIdx.x + 1] = s1;
}

// dw[n][ch * HW + cell] = slab 0 + slab 1 + .. at [n][cell * 32 + ch]: block (cell block of 32, n) reads 1024 consecutive floats of each
// slab and writes 32 runs of 32 cells.  The blocks past the weight's add the bias gradient's partial rows.
__global__ __launch_bounds__(256) void pmx_head_wgrad_sum_kernel(const float *__restrict__ slab, const float *__restrict__ partial, float *__restrict__ dw,
                                                                float *__restrict__ db, int HW, int n_slabs, int db_rows, int cell_blocks)
{
    __shared__ float t[32][33];
    const int K = 32 * HW;
    if ((int)blockIdx.x >= cell_blocks * HID) {
        const int n = (blockIdx.x - cell_blocks * HID) * 256 + threadIdx.x;
        float s = 0.f;
        for (int p = 0; p < db_rows; ++p) s += partial[p * HID + n];
        db[n] = s;
        return;
    }
    const int n = blockIdx.x / cell_blocks, cell0 = (blockIdx.x % cell_blocks) * 32;
    const int k = cell0 * 32 + 4 * threadIdx.x;
    float4 s = float4{0.f, 0.f, 0.f, 0.f};
    if (k < K) {
        s = *reinterpret_cast<const float4 *>(slab + (size_t)n * K + k);
        for (int c = 1; c < n_slabs; ++c) {
            const float4 v = *reinterpret_cast<const float4 *>(slab + ((size_t)c * HID + n) * K + k);
            s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
        }
    }
    const int cl = threadIdx.x >> 3, ch = (threadIdx.x & 7) * 4;
    t[cl][ch] = s.x, t[cl][ch + 1] = s.y, t[cl][ch + 2] = s.z, t[cl][ch + 3] = s.w;
    __syncthreads();
    const int c_out = threadIdx.x & 31;
    if (cell0 + c_out < HW)
        for (int c = threadIdx.x >> 5; c < 32; c += 8) dw[(size_t)n * K + (size_t)c * HW + cell0 + c_out] = t[c_out][c];
}

// Wp from the float32 parameter, every value rounded once: block (64 cells, 8 output features) reads 256-byte runs of cells and writes
// 4 KiB runs of (cell, channel).  LDS rows of 34 bf16 (17 words): the 16-bit stores of a wave (consecutive cells) and its 32-bit reads
// fall on distinct banks.
__global__ __launch_bounds__(256) void pmx_head_pack_kernel(const float *__restrict__ w, unsigned short *__restrict__ wp, int HW, int Kp)
{
    __shared__ __attribute__((aligned(4))) unsigned short t[8 * 64][34];
    const int K = 32 * HW, cell0 = blockIdx.x * 64, n0 = blockIdx.y * 8;
    for (int e = threadIdx.x; e < 8 * 32 * 64; e += 256) {
        const int cl = e & 63, ch = (e >> 6) & 31, nl = e >> 11, cell = cell0 + cl;
        t[nl * 64 + cl][ch] = cell < HW ? bf_one(w[(size_t)(n0 + nl) * K + (size_t)ch * HW + cell]) : (unsigned short)0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 8 * 64 * 16; e += 256) {
        const int cp = e & 15, cl = (e >> 4) & 63, nl = e >> 10, cell = cell0 + cl;
        if (cell * 32 < Kp)
            *reinterpret_cast<uint32_t *>(wp + (size_t)(n0 + nl) * Kp + cell * 32 + 2 * cp) = *reinterpret_cast<const uint32_t *>(&t[nl * 64 + cl][2 * cp]);
    }
}

// WpT [K][512] from Wp [512][Kp]: 64 x 64 tiles, 128-byte runs both ways
__global__ __launch_bounds__(256) void pmx_head_pack_t_kernel(const unsigned short *__restrict__ wp, unsigned short *__restrict__ wpt, int K, int Kp)
{
    __shared__ __attribute__((aligned(4))) unsigned short t[64][66];
    const int k0 = blockIdx.x * 64, n0 = blockIdx.y * 64;                    // (Kp is a multiple of 64: every read is inside Wp)
    for (int e = threadIdx.x; e < 64 * 32; e += 256) {
        const int kp = e & 31, nl = e >> 5;
        *reinterpret_cast<uint32_t *>(&t[nl][2 * kp]) = *reinterpret_cast<const uint32_t *>(wp + (size_t)(n0 + nl) * Kp + k0 + 2 * kp);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * 32; e += 256) {
        const int np = e & 31, kl = e >> 5;
        if (k0 + kl < K)
            *reinterpret_cast<uint32_t *>(wpt + (size_t)(k0 + kl) * HID + n0 + 2 * np) = (uint32_t)t[2 * np][kl] | ((uint32_t)t[2 * np + 1][kl] << 16);
    }
}

struct HeadPlan {
    int K, Kp, ksteps;
    int tiles_m, splits, steps_per_split;          // forward
    int tiles_k, chunks, steps_per_chunk;          // weight gradient
    int db_rows, db_rows_per_block;
    int64_t fwd_bytes, slab_bytes, bwd_bytes;
};

int64_t fwd_scratch_bound(int ksteps, int64_t B)
{
    // the forward slabs hold splits * B rows with splits <= min(ksteps, FWD_MAX_SPLIT) and, when split at all, splits * tiles_m <= FWD_BLOCKS / 4:
    // at most 128 * FWD_BLOCKS / 4 rows.  The bound is monotone in B, which the exact figure is not.
    const int64_t smax = ksteps < FWD_MAX_SPLIT ? ksteps : FWD_MAX_SPLIT;
    const int64_t rows = smax * B < (int64_t)TILE * FWD_BLOCKS / 4 ? smax * B : (int64_t)TILE * FWD_BLOCKS / 4;
    return rows * HID * (int64_t)sizeof(float);
}

HeadPlan plan_for(int H, int W, int64_t B)
{
    HeadPlan p;
    p.K = 32 * H * W;
    p.Kp = (p.K + BK - 1) / BK * BK;
    p.ksteps = p.Kp / BK;
    p.tiles_m = (int)((B + TILE - 1) / TILE);
    int s = p.tiles_m > 0 ? FWD_BLOCKS / (4 * p.tiles_m) : 1;
    s = s < 1 ? 1 : s > FWD_MAX_SPLIT ? FWD_MAX_SPLIT : s;
    s = s > p.ksteps ? p.ksteps : s;
    p.steps_per_split = (p.ksteps + s - 1) / s;
    p.splits = (p.ksteps + p.steps_per_split - 1) / p.steps_per_split;
    p.fwd_bytes = fwd_scratch_bound(p.ksteps, B);
    p.tiles_k = (p.K + TILE - 1) / TILE;
    const int nsteps = (int)((B + BK - 1) / BK);
    int c = WG_BLOCKS / (4 * p.tiles_k);
    c = c < 1 ? 1 : c;
    c = c > nsteps ? nsteps : c;
    p.steps_per_chunk = c > 0 ? (nsteps + c - 1) / c : 1;
    p.chunks = c > 0 ? (nsteps + p.steps_per_chunk - 1) / p.steps_per_chunk : 0;
    p.slab_bytes = (int64_t)c * HID * p.K * (int64_t)sizeof(float);           // c, not chunks: monotone in B
    p.db_rows_per_block = (int)((B + DB_ROWS - 1) / DB_ROWS);
    p.db_rows = p.db_rows_per_block > 0 ? (int)((B + p.db_rows_per_block - 1) / p.db_rows_per_block) : 0;
    p.bwd_bytes = p.slab_bytes + (int64_t)DB_ROWS * HID * (int64_t)sizeof(float);
    return p;
}

constexpr int64_t MAX_B = PMX_ACTOR_HEAD_MAX_BATCH;     // row indices and grid sizes stay far inside 32 bits

int check_board(int32_t H, int32_t W, int64_t B)
{
    if (B < 0) return PMX_ERR_INVALID;
    if (!pmx_actor_supported(H, W) || B > MAX_B) return PMX_ERR_UNSUPPORTED;
    return PMX_OK;
}

}   // namespace

// ---------------------------------------------------------------------------------------------------------------
// C ABI (pacman_mappo_resnet.py:117-119)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int pmx_actor_head_sizes(int32_t H, int32_t W, int64_t B, int64_t *pack_bytes, int64_t *scratch_bytes)
{
    const int rc = check_board(H, W, B);
    if (rc) return rc;
    const HeadPlan p = plan_for(H, W, B);
    if (pack_bytes) *pack_bytes = (int64_t)HID * p.Kp * 2 + (int64_t)p.K * HID * 2;
    if (scratch_bytes) *scratch_bytes = p.fwd_bytes > p.bwd_bytes ? p.fwd_bytes : p.bwd_bytes;
    return PMX_OK;
}

extern "C" int pmx_actor_head_pack(const float *w, void *pack_dev, int32_t H, int32_t W, void *stream)
{
    if (!w || !pack_dev) return PMX_ERR_INVALID;
    const int rc = check_board(H, W, 0);
    if (rc) return rc;
    const HeadPlan p = plan_for(H, W, 0);
    unsigned short *wp = reinterpret_cast<unsigned short *>(pack_dev), *wpt = wp + (size_t)HID * p.Kp;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pmx_head_pack_kernel, dim3((p.Kp / 32 + 63) / 64, HID / 8), dim3(256), 0, st, w, wp, (int)(H * W), p.Kp);
    hipLaunchKernelGGL(pmx_head_pack_t_kernel, dim3(p.Kp / 64, HID / 64), dim3(256), 0, st, (const unsigned short *)wp, wpt, p.K, p.Kp);
    return pmx_launch_rc();
}

extern "C" int pmx_actor_head_forward(const void *feat_dev, const void *pack_dev, const float *bias, void *h_dev, void *scratch_dev, int64_t B,
                                      int32_t H, int32_t W, void *stream)
{
    const int rc = check_board(H, W, B);
    if (rc) return rc;
    if (B == 0) return PMX_OK;
    if (!feat_dev || !pack_dev || !bias || !h_dev || !scratch_dev) return PMX_ERR_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const HeadPlan p = plan_for(H, W, B);
    const char *feat = reinterpret_cast<const char *>(feat_dev), *wp = reinterpret_cast<const char *>(pack_dev);
    const int blocks = p.tiles_m * 4 * p.splits;
    if (p.splits == 1) {
        hipLaunchKernelGGL(pmx_head_gemm_nt_kernel<1>, dim3(blocks), dim3(256), 0, st, feat, wp, bias, h_dev, (int)B, HID, p.K * 2, p.Kp * 2, p.K / 8,
                           p.ksteps, p.steps_per_split, p.tiles_m, 4);
    } else {
        hipLaunchKernelGGL(pmx_head_gemm_nt_kernel<0>, dim3(blocks), dim3(256), 0, st, feat, wp, (const float *)nullptr, scratch_dev, (int)B, HID, p.K * 2,
                           p.Kp * 2, p.K / 8, p.ksteps, p.steps_per_split, p.tiles_m, 4);
        const int64_t quads = B * (HID / 4);
        hipLaunchKernelGGL(pmx_head_fwd_sum_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, (const float *)scratch_dev, bias,
                           (unsigned short *)h_dev, quads, B * HID, p.splits);
    }
    return pmx_launch_rc();
}

extern "C" int pmx_actor_head_backward(const void *feat_dev, const void *dh_dev, const void *pack_dev, void *dfeat_dev, float *dw_dev, float *db_dev,
                                       void *scratch_dev, int64_t B, int32_t H, int32_t W, void *stream)
{
    const int rc = check_board(H, W, B);
    if (rc) return rc;
    if (B == 0) return PMX_OK;
    if (!feat_dev || !dh_dev || !pack_dev || !dfeat_dev || !dw_dev || !db_dev || !scratch_dev) return PMX_ERR_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const HeadPlan p = plan_for(H, W, B);
    const char *feat = reinterpret_cast<const char *>(feat_dev), *dh = reinterpret_cast<const char *>(dh_dev);
    const char *wpt = reinterpret_cast<const char *>(pack_dev) + (size_t)HID * p.Kp * 2;
    // dfeat[B][K] = dh[B][512] . WpT[K][512]^T
    hipLaunchKernelGGL(pmx_head_gemm_nt_kernel<1>, dim3(p.tiles_m * p.tiles_k), dim3(256), 0, st, dh, wpt, (const float *)nullptr, dfeat_dev, (int)B, p.K,
                       HID * 2, HID * 2, HID / 8, HID / BK, HID / BK, p.tiles_m, p.tiles_k);
    float *slab = reinterpret_cast<float *>(scratch_dev), *partial = reinterpret_cast<float *>(reinterpret_cast<char *>(scratch_dev) + p.slab_bytes);
    hipLaunchKernelGGL(pmx_head_wgrad_kernel, dim3(p.tiles_k * 4 * p.chunks), dim3(256), 0, st, dh, feat, slab, (int)B, p.K, p.steps_per_chunk, p.tiles_k);
    hipLaunchKernelGGL(pmx_head_db_partial_kernel, dim3(p.db_rows), dim3(256), 0, st, (const uint32_t *)dh_dev, partial, (int)B, p.db_rows_per_block);
    const int cell_blocks = (H * W + 31) / 32;
    hipLaunchKernelGGL(pmx_head_wgrad_sum_kernel, dim3(cell_blocks * HID + HID / 256), dim3(256), 0, st, (const float *)slab, (const float *)partial, dw_dev,
                       db_dev, (int)(H * W), p.chunks, p.db_rows, cell_blocks);
    return pmx_launch_rc();
}
