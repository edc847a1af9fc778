// style_edit.hip — the edited style vectors of the counterfactual experiment (attfind.counterfactual_images), one launch.
//
// Reference: stylex/FID_TensorFlow.ipynb cell 20 (create_counterfactual_dataset).  For every latent the notebook walks the
// first k (direction, coordinate) pairs of the ranked list, recomputes the style vector, adds
// (target - current) * shift to one bias, and runs the generator; the target is the coordinate's minimum or maximum over
// the dataset, the direction swapped for an image of class 0.  Because the vector is recomputed after every bias
// mutation the edits are SEQUENTIAL: a coordinate that is listed twice moves from its already moved value.
//
// Here: out(l, n, c) for L levels (level l = the first level_k[l] pairs), N images and S coordinates.  One thread owns one
// output element: it reads coords[n][c], walks the first level_k[l] list entries in list order (the list sits in LDS) and
// applies those that name its column, then stores the value once.  No thread reads what another writes, so the launch
// geometry cannot enter the result.  The shift is three separately rounded fp32 operations, target - v, times shift, plus v
// (contraction off): the bits of the torch composition  delta = (target - s) * shift; s += delta.
//
// Output layout, segment-major: segment g = columns seg_start[g] .. seg_start[g + 1] - 1 is a dense [L][N][w_g] tensor at
// float offset L * N * seg_start[g]; the segments are the generator blocks' (style1, style2) widths, so a block's style
// tensor at one level is a contiguous view.
//
// One element per thread and one multiply per element: there are no rows of independent scalar products for the SLP
// vectoriser to pair (the pattern torgb.hip, fid.hip and bn_train.hip are built without it for), so this file takes the
// default flags.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stylex_internal.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_K = 64;  // list entries kept in LDS; the notebook's table has 10

__device__ __forceinline__ float shifted(float v, float target, float shift) {
#pragma clang fp contract(off)
    const float d = target - v;
    const float m = d * shift;
    return v + m;
}

__global__ __launch_bounds__(NT) void style_edit_levels_kernel(
    const float* __restrict__ coords, const float* __restrict__ smin, const float* __restrict__ smax,
    const int* __restrict__ sindex, const int* __restrict__ direction, const int* __restrict__ base_class,
    const int* __restrict__ level_k, const int* __restrict__ seg_start, float* __restrict__ out, int N, int S, int K, int G,
    long total, float shift) {
    __shared__ int s_idx[MAX_K], s_dir[MAX_K];
    const int tid = threadIdx.x;
    if (tid < K) {
        s_idx[tid] = sindex[tid];
        s_dir[tid] = direction[tid];
    }
    __syncthreads();
    const int row = blockIdx.x;  // l * N + n
    const int l = row / N, n = row - l * N;
    const int c = blockIdx.y * NT + tid;
    if (c >= S) return;
    const int kl = min(max(level_k[l], 0), K);
    const bool flip = base_class[n] == 0;
    float v = coords[(long)n * S + c];
    for (int j = 0; j < kl; ++j) {
        if (s_idx[j] != c) continue;
        const bool towards_min = (s_dir[j] == 0) != flip;
        v = shifted(v, towards_min ? smin[c] : smax[c], shift);
    }
    // the segment of column c: the last g with seg_start[g] <= c
    int lo = 0, hi = G;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_start[mid] <= c) lo = mid;
        else hi = mid;
    }
    const int s0 = seg_start[lo], w = seg_start[lo + 1] - s0;
    const long off = (long)gridDim.x * s0 + (long)row * w + (c - s0);
    // a table that breaks its contract (checked by the caller on the host) must not turn into a write outside the buffer
    if (c >= s0 && c - s0 < w && off >= 0 && off < total) out[off] = v;
}

}  // namespace

extern "C" {

int64_t stylex_style_edit_max_k(void) { return MAX_K; }

int stylex_style_edit_levels(const float* coords, const float* smin, const float* smax, const int32_t* sindex,
                             const int32_t* direction, const int32_t* base_class, const int32_t* level_k,
                             const int32_t* seg_start, float* out, int64_t N, int64_t S, int64_t K, int64_t L, int64_t G,
                             float shift_size, void* stream) {
    if (!coords || !smin || !smax || !sindex || !direction || !base_class || !level_k || !seg_start || !out) return STYLEX_EINVAL;
    if (N < 1 || S < 1 || K < 1 || L < 1 || G < 1 || K > MAX_K || G > S) return STYLEX_EINVAL;
    // grid: x = L * N rows, y = column chunks; offsets in 64 bits
    if (N > 0x7fffffff || L > 0x7fffffff || L * N > 0x7fffffff || S > 65535ll * NT || L * N > (1ll << 62) / S) return STYLEX_EINVAL;
    stylex_note_kernel("style_edit_levels_kernel");
    hipLaunchKernelGGL(style_edit_levels_kernel, dim3((unsigned)(L * N), (unsigned)((S + NT - 1) / NT)), dim3(NT), 0,
                       (hipStream_t)stream, coords, smin, smax, sindex, direction, base_class, level_k, seg_start, out, (int)N,
                       (int)S, (int)K, (int)G, (long)(L * N * S), shift_size);
    return (int)hipGetLastError();
}

}  // extern "C"
