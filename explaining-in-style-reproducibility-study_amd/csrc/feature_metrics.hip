// feature_metrics.hip — the pairwise passes over pooled Inception features behind KID and improved precision / recall
// (stylex/fid.py: kid, precision_recall).  Several small kernels with one job each; no atomics anywhere, so the
// same inputs give the same bits; nothing of size n x m is ever held beyond one row block.
//
//   rownorm_f64_kernel       nx[i] = sum_k x[i][k]^2 in fp64, one wave per row
//   pair_f64_kernel<POLY>    per 16 x 16 tile of the n x m pairs: dot products on v_mfma_f64_16x16x4_f64, the polynomial
//                            kernel (dot * gamma + coef0)^3 per pair, ONE fp64 sum per tile -> tile_sums[ti][tj]
//   pair_f64_kernel<DIST2>   the same dot products, max(nx[i] + ny[j] - 2 dot, 0) written to a row block [R][m]
//   sum_f64_kernel           the sum of the tile sums, one block, one fixed order
//   row_kth_smallest_kernel  the k-th smallest entry of every row of a DIST2 block (own column left out by index)
//   col_any_within_kernel    flag[j] |= any_i d2[i][j] <= r2[row0 + i]: one owner per column and launch
// Built without the SLP vectoriser (Makefile: CXXFLAGS_feature_metrics), the rule of torgb.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stylex_internal.h"

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

enum { POLY = 0, DIST2 = 1 };

// Fixed-shape butterfly over the 64 lanes of a wave: every lane ends with the same value, the same order every run.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}

// nx[i] = x[i][0]^2 + ... : lane l adds k = 4 l + 256 q + {0..3} (q ascending), then the butterfly.
__global__ __launch_bounds__(256) void rownorm_f64_kernel(const float* __restrict__ x, double* __restrict__ nx, unsigned n, unsigned D) {
    const unsigned row = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= n) return;  // whole waves leave
    const unsigned lane = threadIdx.x & 63u;
    const float* p = x + row * D;
    double acc = 0.0;
    for (unsigned k = lane * 4u; k < D; k += 256u) {
        const float4 q = *reinterpret_cast<const float4*>(p + k);
        acc += (double)q.x * (double)q.x;
        acc += (double)q.y * (double)q.y;
        acc += (double)q.z * (double)q.z;
        acc += (double)q.w * (double)q.w;
    }
    acc = wave_sum(acc);
    if (lane == 0u) nx[row] = acc;
}

// One wave per 16 x 16 tile of the pairs (x row xr0 + i, y row j), i < R, j < m; tiles row-major, TJ per row of tiles.
// v_mfma_f64_16x16x4_f64, the mapping documented above fid_gram_kernel (fid.hip): lane l holds A[row l & 15][k = l >> 4]
// and B[k = l >> 4][col l & 15]; result register g of lane l is C[row (l >> 4) + 4 g][col l & 15].  Here A[i][.] is x row
// xr0 + i0 + i and B[.][j] is y row j0 + j, fp32 widened to fp64 on load.  D is walked in ascending blocks of 16: a lane
// loads the four floats k0 + 4 (l >> 4) + {0..3} of its row at once, and MFMA q of the block takes element q of both, so
// A and B always meet at the same k.  Rows past R / m are zeros and are never stored or summed.
//   POLY:  t = dot * gamma + coef0, v = t t t; the tile's valid v (without global i == j when `symmetric`) are added per
//          lane as (g0 + g1) + (g2 + g3), then by the butterfly; lane 0 writes tile_sums[tile].
//   DIST2: out[i][j] = max((nx[xr0 + i] + ny[j]) - 2 dot, 0), out dense [R][m].
template <int MODE>
__global__ __launch_bounds__(256) void pair_f64_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const double* __restrict__ nx, const double* __restrict__ ny,
                                                       double* __restrict__ out, unsigned xr0, unsigned R, unsigned m, unsigned D,
                                                       unsigned TJ, unsigned tiles, int symmetric, double gamma, double coef0) {
    const unsigned t = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (t >= tiles) return;  // whole waves leave: every MFMA below runs with all 64 lanes
    const unsigned lane = threadIdx.x & 63u, col = lane & 15u, kq = lane >> 4;
    const unsigned ti = t / TJ, tj = t - ti * TJ;
    const unsigned i0 = ti * 16u, j0 = tj * 16u;
    const bool a_ok = i0 + col < R, b_ok = j0 + col < m;
    // a row that does not exist reads row 0's address but never loads from it
    const float* pa = x + (a_ok ? (xr0 + i0 + col) * D : 0u) + kq * 4u;
    const float* pb = y + (b_ok ? (j0 + col) * D : 0u) + kq * 4u;
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
    for (unsigned k0 = 0; k0 < D; k0 += 16u) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a_ok) a = *reinterpret_cast<const float4*>(pa + k0);
        if (b_ok) b = *reinterpret_cast<const float4*>(pb + k0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.x, (double)b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.y, (double)b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.z, (double)b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.w, (double)b.w, acc, 0, 0, 0);
    }
    const unsigned j = j0 + col;
    if (MODE == POLY) {
        double v[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const unsigned i = i0 + kq + 4u * g;
            const double tt = acc[g] * gamma + coef0;
            const bool keep = i < R && j < m && !(symmetric && xr0 + i == j);
            v[g] = keep ? tt * tt * tt : 0.0;
        }
        const double s = wave_sum((v[0] + v[1]) + (v[2] + v[3]));
        if (lane == 0u) out[t] = s;
    } else {
        if (j < m) {
            const double nyj = ny[j];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const unsigned i = i0 + kq + 4u * g;
                if (i < R) out[i * m + j] = fmax((nx[xr0 + i] + nyj) - 2.0 * acc[g], 0.0);
            }
        }
    }
}

// out[0] = sum of v[0 .. count): thread t adds v[t], v[t + 256], ... ascending, then a fixed tree over the 256 partials.
__global__ __launch_bounds__(256) void sum_f64_kernel(const double* __restrict__ v, double* __restrict__ out, unsigned count) {
    __shared__ double part[256];
    double acc = 0.0;
    for (unsigned i = threadIdx.x; i < count; i += 256u) acc += v[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (unsigned s = 128u; s >= 1u; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0u) out[0] = part[0];
}

// r2[row] = k-th smallest of block[row][j], j != self0 + row (when self0 >= 0).  One wave per row: every lane keeps the 8
// smallest of its columns (j = lane, lane + 64, ...) as a sorted list in registers; then k rounds take the wave's smallest
// list head away from the lowest lane that holds it.  Equal values are separate entries; which of them goes first does not
// change the k-th value.  The host guarantees at least k columns besides the skipped one.
__global__ __launch_bounds__(256) void row_kth_smallest_kernel(const double* __restrict__ block, double* __restrict__ r2, unsigned R,
                                                               unsigned M, int k, int self0) {
    const unsigned row = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= R) return;  // whole waves leave
    const unsigned lane = threadIdx.x & 63u;
    const double inf = __builtin_huge_val();
    double a0 = inf, a1 = inf, a2 = inf, a3 = inf, a4 = inf, a5 = inf, a6 = inf, a7 = inf;
    const double* p = block + row * M;
    const unsigned skip = self0 >= 0 ? (unsigned)self0 + row : 0xffffffffu;
    for (unsigned j = lane; j < M; j += 64u) {
        if (j == skip) continue;
        double v = p[j], w;
        // insertion into the ascending list: the larger of each pair moves on
        w = fmax(a0, v); a0 = fmin(a0, v); v = w;
        w = fmax(a1, v); a1 = fmin(a1, v); v = w;
        w = fmax(a2, v); a2 = fmin(a2, v); v = w;
        w = fmax(a3, v); a3 = fmin(a3, v); v = w;
        w = fmax(a4, v); a4 = fmin(a4, v); v = w;
        w = fmax(a5, v); a5 = fmin(a5, v); v = w;
        w = fmax(a6, v); a6 = fmin(a6, v); v = w;
        a7 = fmin(a7, v);
    }
    double kth = inf;
    for (int r = 0; r < k; ++r) {
        kth = wave_min(a0);
        const unsigned long long holders = __ballot(a0 == kth);
        if (holders != 0ull && lane == (unsigned)(__ffsll((long long)holders) - 1)) {
            a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = a5; a5 = a6; a6 = a7; a7 = inf;
        }
    }
    if (lane == 0u) r2[row] = kth;
}

// flags[j] |= any_i block[i][j] <= r2[row0 + i].  A block of 256 threads owns 64 columns: thread (c, g) looks at rows
// g, g + 4, ...; the four answers meet in LDS and thread (c, 0) alone reads and writes flags[j].
__global__ __launch_bounds__(256) void col_any_within_kernel(const double* __restrict__ block, const double* __restrict__ r2,
                                                             unsigned char* __restrict__ flags, unsigned row0, unsigned R, unsigned M) {
    __shared__ unsigned char hit[4][64];
    const unsigned c = threadIdx.x & 63u, g = threadIdx.x >> 6;
    const unsigned j = blockIdx.x * 64u + c;
    unsigned char any = 0;
    if (j < M)
        for (unsigned i = g; i < R; i += 4u) any |= block[i * M + j] <= r2[row0 + i] ? 1 : 0;
    hit[g][c] = any;
    __syncthreads();
    if (g == 0u && j < M) {
        const unsigned char all = hit[0][c] | hit[1][c] | hit[2][c] | hit[3][c];
        flags[j] = (flags[j] | all) ? 1 : 0;
    }
}

const int64_t IMAX = 0x7fffffffLL;

inline bool bad_dim(int64_t D) { return D < 16 || D % 16 != 0 || D > IMAX; }
inline bool mis(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
inline int64_t tiles16(int64_t n) { return (n + 15) / 16; }

}  // namespace

extern "C" {

int stylex_feat_rownorm(const float* x, double* out, int64_t n, int64_t D, void* stream) {
    if (!x || !out || n < 1 || bad_dim(D) || n > IMAX || n * D > IMAX) return STYLEX_EINVAL;
    if (mis(x, 15) || mis(out, 7)) return STYLEX_EINVAL;
    hipLaunchKernelGGL(rownorm_f64_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, out, (unsigned)n,
                       (unsigned)D);
    return (int)hipGetLastError();
}

int64_t stylex_feat_poly_workspace_bytes(int64_t n, int64_t m) {
    if (n < 1 || m < 1 || n > IMAX || m > IMAX) return -1;
    const int64_t tiles = tiles16(n) * tiles16(m);
    if (tiles > IMAX - 3) return -1;
    return tiles * 8;
}

int stylex_feat_poly_sum(const float* x, const float* y, int64_t n, int64_t m, int64_t D, int symmetric, double gamma, double coef0,
                         double* tile_sums_ws, double* out, void* stream) {
    if (!x || !y || !tile_sums_ws || !out || bad_dim(D)) return STYLEX_EINVAL;
    const int64_t ws = stylex_feat_poly_workspace_bytes(n, m);
    if (ws < 0 || n * D > IMAX || m * D > IMAX) return STYLEX_EINVAL;
    if (symmetric && n != m) return STYLEX_EINVAL;
    if (mis(x, 15) || mis(y, 15) || mis(tile_sums_ws, 7) || mis(out, 7)) return STYLEX_EINVAL;
    const int64_t TJ = tiles16(m), tiles = ws / 8;
    hipLaunchKernelGGL(pair_f64_kernel<POLY>, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y,
                       (const double*)nullptr, (const double*)nullptr, tile_sums_ws, 0u, (unsigned)n, (unsigned)m, (unsigned)D,
                       (unsigned)TJ, (unsigned)tiles, symmetric ? 1 : 0, gamma, coef0);
    hipLaunchKernelGGL(sum_f64_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)tile_sums_ws, out, (unsigned)tiles);
    return (int)hipGetLastError();
}

int stylex_feat_dist2_block(const float* x, const float* y, const double* nx, const double* ny, int64_t row0, int64_t R, int64_t n,
                            int64_t m, int64_t D, double* out_block, void* stream) {
    if (!x || !y || !nx || !ny || !out_block || bad_dim(D)) return STYLEX_EINVAL;
    if (n < 1 || m < 1 || n > IMAX || m > IMAX || n * D > IMAX || m * D > IMAX) return STYLEX_EINVAL;
    if (row0 < 0 || R < 1 || row0 > n || R > n - row0 || R * m > IMAX) return STYLEX_EINVAL;
    if (mis(x, 15) || mis(y, 15) || mis(nx, 7) || mis(ny, 7) || mis(out_block, 7)) return STYLEX_EINVAL;
    const int64_t TJ = tiles16(m), tiles = tiles16(R) * TJ;
    if (tiles > IMAX - 3) return STYLEX_EINVAL;
    hipLaunchKernelGGL(pair_f64_kernel<DIST2>, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y, nx, ny,
                       out_block, (unsigned)row0, (unsigned)R, (unsigned)m, (unsigned)D, (unsigned)TJ, (unsigned)tiles, 0, 0.0, 0.0);
    return (int)hipGetLastError();
}

int stylex_feat_row_kth(const double* block, int64_t R, int64_t M, int64_t k, int64_t self0, double* out_r2, void* stream) {
    if (!block || !out_r2 || R < 1 || M < 1 || R > IMAX || M > IMAX || R * M > IMAX) return STYLEX_EINVAL;
    if (k < 1 || k > 8) return STYLEX_EINVAL;
    if (self0 >= 0 && (self0 > M || R > M - self0)) return STYLEX_EINVAL;  // every row's own column lies inside the block
    if (k > M - (self0 >= 0 ? 1 : 0)) return STYLEX_EINVAL;                // a symmetric call needs k < n neighbours
    if (mis(block, 7) || mis(out_r2, 7)) return STYLEX_EINVAL;
    hipLaunchKernelGGL(row_kth_smallest_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, block, out_r2,
                       (unsigned)R, (unsigned)M, (int)k, self0 >= 0 ? (int)self0 : -1);
    return (int)hipGetLastError();
}

int stylex_feat_col_any(const double* block, const double* r2, int64_t row0, int64_t R, int64_t M, unsigned char* flags,
                        void* stream) {
    if (!block || !r2 || !flags || R < 1 || M < 1 || R > IMAX || M > IMAX || R * M > IMAX) return STYLEX_EINVAL;
    if (row0 < 0 || row0 > IMAX - R) return STYLEX_EINVAL;
    if (mis(block, 7) || mis(r2, 7)) return STYLEX_EINVAL;
    hipLaunchKernelGGL(col_any_within_kernel, dim3((unsigned)((M + 63) / 64)), dim3(256), 0, (hipStream_t)stream, block, r2, flags,
                       (unsigned)row0, (unsigned)R, (unsigned)M);
    return (int)hipGetLastError();
}

}  // extern "C"
