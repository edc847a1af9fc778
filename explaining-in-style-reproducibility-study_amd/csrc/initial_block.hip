// initial_block.hip — the generator's first activation with no_const (reference stylex_train.py:766-769, :798-802):
//   x = ConvTranspose2d(D, C, 4, 1, 0, bias=False)(styles.mean(dim=1)[:, :, None, None])
// On a 1x1 input the transposed conv is a matrix product: with avg[b][d] = mean_l styles[b][l][d], the weight
// W [D][C][4][4] read as the matrix [D][N], N = 16 C, column n = c * 16 + p (p = 4 i + j),
//   forward          x[b][p][c]      = sum_d avg[b][d] W[d][n]                   (channels-last: offset b N + p C + c)
//   data gradient    dstyles[b][l][d] = (1 / L) sum_n gx[b][p][c] W[d][n]        (the same row for every l)
//   weight gradient  dW[d][n]         = sum_b avg[b][d] gx[b][p][c]
// The op is bilinear in (styles, W); each of its gradients is one of these three launches again (ops.py), which is what the
// path-length step needs.  The mean over L is taken while the styles are read — avg is never a tensor.  fp32 accumulation;
// the weight operand is fp32 or a packed bf16 copy in the same [D][N] order; x / gx are fp32 or bf16.  Every sum runs in
// a fixed order (no atomics): the same inputs give the same bits.  All accesses are per element, so a row length that is
// no multiple of 4 (D = 514) needs no tail handling; rows and columns past the end are guarded.
//
// Traffic: the weight (514 x 8192 at C = 512: 16.8 MB fp32, 8.4 MB bf16) dominates.  Forward and weight gradient give a
// thread one weight column (coalesced rows); a block re-reads its 256-column slice once per tile of 8 samples (forward),
// which the L2 serves — HBM sees the weight once per launch.  The data gradient gives a block 4 weight rows, staged
// through LDS in 64-channel chunks in the order gx is stored, and a wave up to 8 samples.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stylex_internal.h"

namespace {

constexpr int IB_T = 256;        // threads per block
constexpr int IB_DMAX = 1024;    // forward: avg tile [D][8] in LDS (32 KB)
constexpr int IB_CMAX = 512;
constexpr int IB_LMAX = 64;      // data gradient: lane l writes row l
constexpr int IB_FB = 8;         // forward: samples per tile
constexpr int IB_WD = 16;        // weight gradient: rows per block
constexpr int IB_WB = 64;        // weight gradient: samples per LDS tile
constexpr int IB_DD = 4;         // data gradient: rows per block
constexpr int IB_DB = 8;       // data gradient: samples per wave
constexpr int IB_ROW = 65;       // data gradient: LDS stride of one pixel's 64 channels (+1: bank spread of the transposing write)

__device__ __forceinline__ float ib_ld(const void* p, long i, int bf) { return act_ld1(p, i, bf); }

// mean over L of styles[b][.][d]
__device__ __forceinline__ float ib_avg(const float* styles, int b, int d, int L, int D) {
    const float* s = styles + ((long)b * L) * D + d;
    float a = 0.f;
    for (int l = 0; l < L; ++l) a += s[(long)l * D];
    return a / (float)L;
}

__global__ __launch_bounds__(IB_T) void initial_block_fwd_kernel(const float* __restrict__ styles, const void* __restrict__ w,
                                                                 void* __restrict__ x, int B, int L, int D, int C, int wbf, int xbf) {
    __shared__ float4 savg[IB_DMAX * IB_FB / 4];  // [d][8 samples]
    float* sa = reinterpret_cast<float*>(savg);
    const int N = 16 * C;
    const int n = blockIdx.x * IB_T + threadIdx.x;
    const int c = n >> 4, p = n & 15;
    for (int b0 = 0; b0 < B; b0 += IB_FB) {
        __syncthreads();
        for (int e = threadIdx.x; e < D * IB_FB; e += IB_T) {
            const int j = e / D, d = e - j * D;  // d fastest: coalesced style reads
            sa[d * IB_FB + j] = b0 + j < B ? ib_avg(styles, b0 + j, d, L, D) : 0.f;
        }
        __syncthreads();
        if (n >= N) continue;
        float acc[IB_FB];
#pragma unroll
        for (int j = 0; j < IB_FB; ++j) acc[j] = 0.f;
        for (int d = 0; d < D; ++d) {
            const float wv = ib_ld(w, (long)d * N + n, wbf);
            const float4 a0 = savg[d * 2], a1 = savg[d * 2 + 1];
            acc[0] = fmaf(a0.x, wv, acc[0]);
            acc[1] = fmaf(a0.y, wv, acc[1]);
            acc[2] = fmaf(a0.z, wv, acc[2]);
            acc[3] = fmaf(a0.w, wv, acc[3]);
            acc[4] = fmaf(a1.x, wv, acc[4]);
            acc[5] = fmaf(a1.y, wv, acc[5]);
            acc[6] = fmaf(a1.z, wv, acc[6]);
            acc[7] = fmaf(a1.w, wv, acc[7]);
        }
#pragma unroll
        for (int j = 0; j < IB_FB; ++j)
            if (b0 + j < B) act_st1(x, (long)(b0 + j) * N + (long)p * C + c, acc[j], xbf);
    }
}

__global__ __launch_bounds__(IB_T) void initial_block_wgrad_kernel(const float* __restrict__ styles, const void* __restrict__ gx,
                                                                   float* __restrict__ dw, int B, int L, int D, int C, int xbf) {
    __shared__ float4 savg[IB_WB * IB_WD / 4];  // [sample][16 rows]
    float* sa = reinterpret_cast<float*>(savg);
    const int N = 16 * C;
    const int n = blockIdx.x * IB_T + threadIdx.x;
    const int d0 = blockIdx.y * IB_WD;
    const long goff = (long)(n & 15) * C + (n >> 4);
    float acc[IB_WD];
#pragma unroll
    for (int r = 0; r < IB_WD; ++r) acc[r] = 0.f;
    for (int b0 = 0; b0 < B; b0 += IB_WB) {
        const int nb = min(IB_WB, B - b0);
        __syncthreads();
        for (int e = threadIdx.x; e < nb * IB_WD; e += IB_T) {
            const int j = e / IB_WD, r = e - j * IB_WD;
            sa[e] = d0 + r < D ? ib_avg(styles, b0 + j, d0 + r, L, D) : 0.f;
        }
        __syncthreads();
        if (n >= N) continue;
        for (int j = 0; j < nb; ++j) {
            const float g = ib_ld(gx, (long)(b0 + j) * N + goff, xbf);
#pragma unroll
            for (int q = 0; q < IB_WD / 4; ++q) {
                const float4 a = savg[j * (IB_WD / 4) + q];
                acc[4 * q + 0] = fmaf(a.x, g, acc[4 * q + 0]);
                acc[4 * q + 1] = fmaf(a.y, g, acc[4 * q + 1]);
                acc[4 * q + 2] = fmaf(a.z, g, acc[4 * q + 2]);
                acc[4 * q + 3] = fmaf(a.w, g, acc[4 * q + 3]);
            }
        }
    }
    if (n >= N) return;
#pragma unroll
    for (int r = 0; r < IB_WD; ++r)
        if (d0 + r < D) dw[(long)(d0 + r) * N + n] = acc[r];
}

// grid = (ceil(D / 4), ceil(B / 32)); wave v of the block owns samples b0 + v + 4 k, k < 8
__global__ __launch_bounds__(IB_T) void initial_block_dgrad_kernel(const void* __restrict__ gx, const void* __restrict__ w,
                                                                   float* __restrict__ dstyles, int B, int L, int D, int C, int wbf,
                                                                   int xbf) {
    __shared__ float sw[IB_DD * 16 * IB_ROW];  // [row][pixel][64 channels (+1)]
    const int N = 16 * C;
    const int d0 = blockIdx.x * IB_DD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bw = blockIdx.y * (4 * IB_DB) + wave;
    float acc[IB_DB][IB_DD];
#pragma unroll
    for (int k = 0; k < IB_DB; ++k)
#pragma unroll
        for (int r = 0; r < IB_DD; ++r) acc[k][r] = 0.f;
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int cw = min(64, C - c0);
        __syncthreads();
        for (int e = threadIdx.x; e < IB_DD * 1024; e += IB_T) {
            const int r = e >> 10, i = e & 1023, cl = i >> 4, p = i & 15;  // i walks the weight row: column (c0 + cl) * 16 + p
            float v = 0.f;
            if (d0 + r < D && cl < cw) v = ib_ld(w, (long)(d0 + r) * N + (long)c0 * 16 + i, wbf);
            sw[(r * 16 + p) * IB_ROW + cl] = v;
        }
        __syncthreads();
        if (lane >= cw) continue;
#pragma unroll 2
        for (int p = 0; p < 16; ++p) {
            float wv[IB_DD];
#pragma unroll
            for (int r = 0; r < IB_DD; ++r) wv[r] = sw[(r * 16 + p) * IB_ROW + lane];
            const long off = (long)p * C + c0 + lane;
#pragma unroll
            for (int k = 0; k < IB_DB; ++k) {
                const int b = bw + 4 * k;
                if (b < B) {  // wave-uniform
                    const float g = ib_ld(gx, (long)b * N + off, xbf);
#pragma unroll
                    for (int r = 0; r < IB_DD; ++r) acc[k][r] = fmaf(g, wv[r], acc[k][r]);
                }
            }
        }
    }
    const float inv = 1.f / (float)L;
#pragma unroll
    for (int k = 0; k < IB_DB; ++k) {
        const int b = bw + 4 * k;
        if (b >= B) continue;
#pragma unroll
        for (int r = 0; r < IB_DD; ++r) {
            float s = acc[k][r];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);  // every lane holds the sum
            if (lane < L && d0 + r < D) dstyles[((long)b * L + lane) * D + d0 + r] = s * inv;
        }
    }
}

bool ib_shape_ok(const int64_t* s) {
    return s && s[0] >= 1 && s[0] <= 65535 && s[1] >= 1 && s[1] <= IB_LMAX && s[2] >= 1 && s[2] <= IB_DMAX && s[3] >= 1 && s[3] <= IB_CMAX;
}

double ib_bytes(const int64_t* s, int wbf, int xbf) {
    return (double)s[2] * 16 * s[3] * (wbf ? 2 : 4) + (double)s[0] * 16 * s[3] * (xbf ? 2 : 4) + 4.0 * s[0] * s[1] * s[2];
}

}  // namespace

extern "C" {

// shape = {B, L, D, C}
int stylex_initial_block_supported(const int64_t* shape) { return ib_shape_ok(shape) ? 1 : 0; }

int stylex_initial_block_fwd(const float* styles, const void* w, void* x, const int64_t* shape, int w_dtype, int act_dtype, void* stream) {
    if (!styles || !w || !x || !ib_shape_ok(shape) || (w_dtype | act_dtype) & ~1) return STYLEX_EINVAL;
    const int B = (int)shape[0], L = (int)shape[1], D = (int)shape[2], C = (int)shape[3];
    StylexTimedCall tm(0, ib_bytes(shape, w_dtype, act_dtype), (hipStream_t)stream);
    stylex_note_kernel("initial_block_fwd_kernel");
    hipLaunchKernelGGL(initial_block_fwd_kernel, dim3((16 * C + IB_T - 1) / IB_T), dim3(IB_T), 0, (hipStream_t)stream, styles, w, x, B, L, D,
                       C, w_dtype, act_dtype);
    return (int)hipGetLastError();
}

int stylex_initial_block_bwd_data(const void* gx, const void* w, float* dstyles, const int64_t* shape, int w_dtype, int act_dtype,
                                  void* stream) {
    if (!gx || !w || !dstyles || !ib_shape_ok(shape) || (w_dtype | act_dtype) & ~1) return STYLEX_EINVAL;
    const int B = (int)shape[0], L = (int)shape[1], D = (int)shape[2], C = (int)shape[3];
    StylexTimedCall tm(1, ib_bytes(shape, w_dtype, act_dtype), (hipStream_t)stream);
    stylex_note_kernel("initial_block_dgrad_kernel");
    hipLaunchKernelGGL(initial_block_dgrad_kernel, dim3((D + IB_DD - 1) / IB_DD, (B + 4 * IB_DB - 1) / (4 * IB_DB)), dim3(IB_T), 0,
                       (hipStream_t)stream, gx, w, dstyles, B, L, D, C, w_dtype, act_dtype);
    return (int)hipGetLastError();
}

int stylex_initial_block_bwd_weight(const float* styles, const void* gx, float* dw, const int64_t* shape, int act_dtype, void* stream) {
    if (!styles || !gx || !dw || !ib_shape_ok(shape) || act_dtype & ~1) return STYLEX_EINVAL;
    const int B = (int)shape[0], L = (int)shape[1], D = (int)shape[2], C = (int)shape[3];
    StylexTimedCall tm(2, ib_bytes(shape, 0, act_dtype), (hipStream_t)stream);
    stylex_note_kernel("initial_block_wgrad_kernel");
    hipLaunchKernelGGL(initial_block_wgrad_kernel, dim3((16 * C + IB_T - 1) / IB_T, (D + IB_WD - 1) / IB_WD), dim3(IB_T), 0,
                       (hipStream_t)stream, styles, gx, dw, B, L, D, C, act_dtype);
    return (int)hipGetLastError();
}

}  // extern "C"
